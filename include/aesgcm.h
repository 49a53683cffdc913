/*
 * aesgcm.h -- C ABI of libaesgcm_hip.so: MI355X (gfx950) AES-GCM bulk path.
 *
 * This is the drop-in boundary for the hot path of BLu85/AES-GCM-128-192-256-bits.  The reference
 * has no FFI of its own: its software surface is the Python class tb/gcm_model.py:5-51, which
 * forwards every call to pycryptodome (tb/gcm_model.py:18 AES.new(..MODE_GCM..), :22 update,
 * :26 encrypt, :30 decrypt, :35 digest, :44 verify).  Each entry point below names the reference
 * item whose arithmetic it replaces (paths relative to the reference checkout); the Python binding
 * a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++/torch/HIP types in any signature
 *     (a HIP stream is passed as void*; NULL = the context's own stream).
 *   - every function returns AESGCM_OK (0) or a negative AESGCM_E* code; nothing throws or aborts.
 *   - ALL cryptographic arithmetic (key expansion, H, GHASH tables, CTR, GHASH, tag) runs in HIP
 *     kernels on the selected device.  There is no CPU fallback: without a usable HIP device every
 *     compute entry point fails with AESGCM_EHIP.
 *   - the caller owns every buffer it passes; the library owns only opaque contexts.
 *   - a context is not thread-safe; distinct contexts may be used from distinct threads.  Calls on ONE
 *     context must be stream-ordered (same stream, or the caller synchronises between streams): a context
 *     owns one set of scratch buffers (two streams driving aesgcm_shard_crypt_dev on ONE context would corrupt
 *     each other's GHASH scratch).  The batch entry points have no context; launches on different streams may
 *     overlap, up to 256 of them in flight per device (each takes the next slot of a 256-entry ring of packet
 *     dispensers, zeroed on its own stream).
 *   - IV is always 96 bits (src/gcm_pkg.vhd:15-17, tb/gcm_gctr.py:251); tag is the full 128 bits
 *     (src/gcm_ghash.vhd:293).
 *   - length rule: data <= 2^36 - 32 bytes (the 32-bit block counter stops at all-ones,
 *     src/aes_icb.vhd:114) and AAD blocks + data blocks < 2^36 -> AESGCM_ETOOLONG otherwise.
 */
#ifndef AESGCM_H
#define AESGCM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AESGCM_ABI_VERSION 5   /* (additions since, the version unchanged: key tables, their frames in wire format, aesgcm_wire_xfmt / aesgcm_keytab_set_xpn / aesgcm_keytab_frames_crypt_x_dev,
                                  aesgcm_tls_fmt / aesgcm_keytab_set_tls_iv / aesgcm_keytab_records_crypt_dev, aesgcm_keytab_quic_crypt_dev,
                                  aesgcm_dtls_fmt / aesgcm_keytab_dtls_crypt_dev, aesgcm_srtp_fmt / aesgcm_keytab_srtp_crypt_dev, the receive windows aesgcm_rxwin_*,
                                  the send counters aesgcm_txnum_* / aesgcm_txnum_fmt, the on-device key derivation aesgcm_kdf_* / aesgcm_kdf_fmt,
                                  SRTP's on-device key derivation aesgcm_srtp_kdf_*, the TLS 1.2 PRF aesgcm_prf12_*, IKEv2's prf+ aesgcm_prfplus_*,
                                  MACsec's MKA aesgcm_mka_*, SSH packets aesgcm_keytab_ssh_crypt_dev, SSH's key derivation aesgcm_sshkdf_*)
                                  5 (round 6): calls with offset arrays and aesgcm_messages_crypt_dev are ROUTED per message on the device (AESGCM_SHAPE_MIXED; pkt_len is no longer a hint),
                                  aesgcm_ctx_status (what an asynchronous call could not say when it returned), aesgcm_stream_export / _import / _update_dev, aesgcm_frames_ceiling_probe_dev,
                                  aesgcm_mgpu_last_tags collects the OLDEST queued messages;
                                  4 (round 5): packets of message size by rows (AESGCM_SHAPE_ROWS), aesgcm_messages_crypt_dev, aesgcm_ctx_last_launch, aesgcm_wipe_failed_dev and the option "wipe_on_auth_fail",
                                  aesgcm_mgpu_crypt_dev with tag = NULL + aesgcm_mgpu_last_tags / aesgcm_mgpu_sync;
                                  2: aesgcm_ctx_wait, aesgcm_comm_* / aesgcm_mgpu_*, packet and batch entry points; 3: aesgcm_ctx_set_option (the library no longer reads
                                  any environment variable), aesgcm_batch_shape / aesgcm_packets_shape, aesgcm_mgpu_ctx, aesgcm_last_tag through the host slot */

#if defined(__GNUC__)
#define AESGCM_API __attribute__((visibility("default")))
#else
#define AESGCM_API
#endif

#define AESGCM_OK        0
#define AESGCM_EARG     (-1)   /* NULL/invalid argument                                        */
#define AESGCM_EKEYLEN  (-2)   /* key length not 16/24/32 (aes_pkg.vhd:60-63 modes 128/192/256) */
#define AESGCM_EIVLEN   (-3)   /* reserved: IV is fixed at 12 bytes by the signatures            */
#define AESGCM_ETOOLONG (-4)   /* message exceeds the counter space (aes_icb.vhd:114)            */
#define AESGCM_EAUTH    (-5)   /* tag mismatch on decrypt (tb/gcm_model.py:47 ValueError branch) */
#define AESGCM_EHIP     (-6)   /* HIP runtime error / no device; see aesgcm_last_error()         */
#define AESGCM_ENOMEM   (-7)
#define AESGCM_ESTATE   (-8)   /* streaming call out of order (AAD after data, ragged chunk)     */
#define AESGCM_EALIGN   (-9)   /* device data pointer not 16-byte aligned                        */
#define AESGCM_ERCCL    (-10)  /* RCCL missing or a collective failed; see aesgcm_comm_last_error() */

typedef struct aesgcm_ctx aesgcm_ctx;

/* ---------------------------------------------------------------- library / device */
AESGCM_API int         aesgcm_abi_version(void);
AESGCM_API const char *aesgcm_strerror(int code);
AESGCM_API const char *aesgcm_last_error(void);              /* thread-local detail of the last AESGCM_EHIP */
AESGCM_API int         aesgcm_device_count(int *n);
AESGCM_API int         aesgcm_device_name(int device, char *buf, size_t buflen);

/* ---------------------------------------------------------------- unit-level entry points
 * One per arithmetic block of the RTL so that each can be parity-tested in isolation.  All run
 * on the GPU (small kernels), results are copied back to the host buffers given. */

/* FIPS-197 KeyExpansion.  Replaces aes_kexp (config/config_aes_kexp.py:113-159, window update
 * :189-219) and its software twin tb/key_exp.py:79-121 aes_expand_key.  rk receives
 * 16*(nr+1) bytes, stage i = bytes 16i..16i+15 (the layout load_pre_exp_key streams,
 * tb/gcm_gctr.py:199-207); *nr = 10/12/14 (aes_pkg.vhd:31-33). */
AESGCM_API int aesgcm_key_expand(int device, const uint8_t *key, size_t key_len, uint8_t rk[240], int *nr);

/* nblocks independent ECB encryptions under the context key through the same LDS T-table round
 * code the CTR kernel uses.  Replaces aes_round x Nr + aes_last_round
 * (config/config_aes_round.py:120-126, src/aes_last_round.vhd:76) as instantiated by aes_ecb
 * (config/config_aes_ecb.py:250-327). */
AESGCM_API int aesgcm_ecb_encrypt(aesgcm_ctx *ctx, const uint8_t *in, size_t nblocks, uint8_t *out);

/* n independent GF(2^128) products z[i] = x[i] * h[i] (16-byte big-endian blocks, GCM bit order).
 * Replaces ghash_gfmul (src/ghash_gfmul.vhd:37-64). */
AESGCM_API int aesgcm_gfmul(int device, const uint8_t *h, const uint8_t *x, uint8_t *z, size_t n);

/* GHASH chaining value after absorbing `len` bytes (last block zero-padded) from Y = 0 under the
 * context's H = E_K(0^128):  Y_i = (Y_{i-1} xor X_i) * H  (src/gcm_ghash.vhd:174-186, :259-272),
 * WITHOUT the length block.  Computed by the parallel H-power path, not by serial Horner. */
AESGCM_API int aesgcm_ghash(aesgcm_ctx *ctx, const uint8_t *data, size_t len, uint8_t y[16]);

/* H = E_K(0^128) as latched by gcm_ghash (src/gcm_gctr.vhd:141-144, src/gcm_ghash.vhd:128-139). */
AESGCM_API int aesgcm_get_h(aesgcm_ctx *ctx, uint8_t h[16]);

/* ---------------------------------------------------------------- context
 * A context = (device, expanded key, H, H-power tables, scratch).  Creating it runs the on-GPU key
 * expansion and table build once per key (the RTL's "load key" phase, tb/gcm_gctr.py:144-175). */
AESGCM_API int aesgcm_ctx_create(aesgcm_ctx **out, int device, const uint8_t *key, size_t key_len);
/* Pre-expanded key load path (config/config_aes_kprexp.py:66-106, tb/gcm_gctr.py:180-214):
 * rk = 16*(nr+1) bytes exactly as aesgcm_key_expand / tb/key_exp.py produce them. */
AESGCM_API int aesgcm_ctx_create_preexpanded(aesgcm_ctx **out, int device, const uint8_t *rk, int nr);
/* A new key for an existing context: the reference core's "load key" between frames (tb/gcm_gctr.py:144-175; H is recomputed only then,
 * src/gcm_gctr.vhd:142-144).  The context keeps its stream, scratch, host slot and options; only the key schedule, H and the H-power tables
 * are rebuilt (0.4 ms, half of what destroying the context and creating another costs).  Waits for the context's queued
 * work first; AESGCM_ESTATE inside an open aesgcm_stream_* session. */
AESGCM_API int aesgcm_ctx_rekey(aesgcm_ctx *ctx, const uint8_t *key, size_t key_len);
AESGCM_API int aesgcm_ctx_destroy(aesgcm_ctx *ctx);
AESGCM_API int aesgcm_ctx_device(const aesgcm_ctx *ctx);
/* Which launch structure the context's last whole-message call (aesgcm_encrypt[_dev] / aesgcm_decrypt[_dev]) took.  The library chooses by size and -- for the
 * half shape of the cyclic rows -- by whether another context of the device had a message under way at that moment; benches and profiles report it. */
#define AESGCM_LAUNCH_NONE 0
#define AESGCM_LAUNCH_MAIN 1            /* k_main (+ k_combine): below 64 KiB */
#define AESGCM_LAUNCH_CYCLIC 2          /* one k_body launch of cyclic rows */
#define AESGCM_LAUNCH_CYCLIC_HALF 3     /* ... in its half shape (k_bodyh) */
#define AESGCM_LAUNCH_DEALT 4           /* k_body's dealt chunks (+ k_fold): from 1 GiB */
AESGCM_API int aesgcm_ctx_last_launch(const aesgcm_ctx *ctx, int *shape);
/* Tunables of one context, for tests and profiling scripts; the library reads no environment variable and the defaults are the
 * measured best.  Every value selects between paths that produce the same bytes.  Keys (value >= 0):
 *   "tw"          rows of 64 blocks per chunk of the dealt kernels, 0 = the library's rule
 *   "body_min"    bytes from which a range's aligned middle goes through k_body's dealt chunks (>= 2^60: never, nor cyclic rows)
 *   "cyc_min", "cyc_max"   bytes: ranges in [cyc_min, cyc_max) take k_body's cyclic rows (one launch per message); both 0 = never
 *   "cyc_close"   1: that launch closes the tag itself; 0: k_fold + k_combine behind it
 *   "cyc_half"    whole messages below 80 MiB take the launch in its half shape (256 workgroups of 512 lanes, two per CU), in which one message's
 *                 table staging and closing run beside another's rows: 0 never, 1 always, 2 (default) when another context of the device has a
 *                 message under way at the moment of the call (its host slot does not yet show its last launch) -- i.e. for callers that keep
 *                 messages in flight on contexts of their own; a single message alone on the chip is slower in that shape
 *   "fold_close"  1: behind the dealt k_body a k_fold level closes the tag; 0: further levels and k_combine
 *   "cyc_prio"    rows between rotations of the waves' issue priorities in a cyclic launch, 0 = off
 *   "pkt_order"   accepted and ignored since round 6 (it was the packet count from which a call with offset arrays took its packets by falling length class: the
 *                 routing sort of such a call makes that order anyway)
 *   "wipe_on_auth_fail"  1: a decrypt call that verifies a tag (expect_tag / d_expect_tags) leaves ZEROS, not unauthenticated plaintext, where verification fails:
 *                 aesgcm_decrypt and aesgcm_decrypt_pipelined wipe the caller's buffer (aesgcm_decrypt does not even copy the plaintext out before the tag is
 *                 checked), aesgcm_decrypt_dev the device buffer, aesgcm_packets_crypt_dev / aesgcm_messages_crypt_dev every packet whose d_auth entry is 0 (d_auth must be given:
 *                 AESGCM_EARG for a decrypt call with d_expect_tags and without d_auth while the option is on).  Default 0:
 *                 the reference model returns the plaintext and raises (tb/gcm_model.py:29-30,47-51), and so does the class that mirrors it.
 *   "rows_min"    bytes per packet from which aesgcm_packets_crypt_dev goes by rows (default 8192; fixed-size records: from a quarter of it while the packets are at most 16384; 0 = never).
 *                 With offset arrays the mark is applied per message on the device, to data + AAD, in steps of 64 bytes and up to 16320 (see "route_mid_min")
 *   "route_mid_min", "route_blocks_min"   how a call with offset arrays is routed on the device: the mark is "rows_min" when at least route_mid_min (65536) of its messages lie
 *                 between a quarter of rows_min and rows_min, else that quarter; and nothing goes to the packet kernels at all while the messages below the mark hold
 *                 fewer than route_blocks_min (2^17) + 3.5 per message 16-byte blocks between them -- unless the call has at most 4096 messages and none above the mark: that is one packet
 *                 launch against three row launches (csrc/aesgcm_kernels.hip route_decide has the measurements).  0 / 0: always the high mark, always split
 *   "route_top_min"   ... and the mark rises to 16320 bytes, the last size the sort resolves, when at least this many messages (458752) lie between "rows_min" and it; 0 = never
 *   "rows_block"  units (rows of 64 blocks) per dealt block of the row kernel, 0 = the library's cut (one block per wave; blocks of 64 for large calls)
 *   "poll_us"     how long a tag is polled for in the pinned host slot before the call blocks in the runtime
 * AESGCM_EARG for an unknown key. */
AESGCM_API int aesgcm_ctx_set_option(aesgcm_ctx *ctx, const char *key, int64_t value);
/* the context's own HIP stream (what `stream = NULL` means everywhere): lets a caller order other work -- the
 * aesgcm_comm_allgather_dev of the partials -- behind the context's kernels without a host synchronisation */
AESGCM_API int aesgcm_ctx_stream(const aesgcm_ctx *ctx, void **stream);
/* Stream-order two contexts of one device without a host synchronisation: what is enqueued on ctx's own stream AFTER this call
 * starts only when everything enqueued on other's own stream BEFORE it has completed.  A context owns one scratch set, so
 * back-to-back messages (the shards of bench.py's N > 1 step) alternate between two contexts of the same key: message m+1's
 * fused kernel then runs while message m's fold / combine kernels drain; the step that consumes both (the all-gather of the
 * partials) is ordered with this call.  No reference counterpart (the RTL has one pipeline, src/aes_gcm.vhd). */
AESGCM_API int aesgcm_ctx_wait(aesgcm_ctx *ctx, aesgcm_ctx *other);
/* The same, but only up to other's most recently enqueued FUSED kernel (the AES-CTR + GHASH launch), not the fold / combine
 * launches behind it: chaining message m+1 (on ctx) to message m (on other) this way runs the fused kernels back to back and
 * lets every fold / combine tail but the last hide behind the next message.  Tracking starts with the first call (which,
 * like any call made before other has launched a fused kernel, waits for nothing). */
AESGCM_API int aesgcm_ctx_wait_fused(aesgcm_ctx *ctx, aesgcm_ctx *other);
/* What an ASYNCHRONOUS call could not say when it returned (round 6).  aesgcm_packets_crypt_dev with offset arrays and aesgcm_messages_crypt_dev read their lengths on the
 * device, behind the call: when the plan kernel finds one it cannot take -- the RTL raises a flag when its counter cannot go on (src/aes_icb.vhd:65,98,114,119) -- NOTHING
 * of that call runs (outputs, tags and d_auth are left as they were) and the reason goes to a status word in the context's pinned host memory, next to its tag slot:
 *   AESGCM_STATUS_LENGTH   a message's data or AAD is 2^28 bytes or more, or an offset array does not rise; *detail = the first such message
 *   AESGCM_STATUS_PLAN     the call's plan does not fit the scratch the library sized for it; *detail = the record slots it asked for
 *   AESGCM_STATUS_UNITS    more rows than 32-bit block numbers hold; *detail = the rows
 * aesgcm_ctx_status reads the word and clears it (no wait: synchronise the stream the call ran on first -- a status is there when that stream has drained); 0 = nothing
 * to report.  While a status is unread, aesgcm_last_tag and aesgcm_ctx_wait on the context return AESGCM_ETOOLONG (LENGTH, UNITS) or AESGCM_ESTATE (PLAN). */
#define AESGCM_STATUS_OK     0
#define AESGCM_STATUS_PLAN   1
#define AESGCM_STATUS_LENGTH 2
#define AESGCM_STATUS_UNITS  3
AESGCM_API int aesgcm_ctx_status(aesgcm_ctx *ctx, int *code, uint64_t *detail);

/* ---------------------------------------------------------------- whole messages, host pointers
 * Replaces the model's update/encrypt/digest sequence (tb/gcm_model.py:21-35) i.e. the aes_gcm
 * top level in encrypt mode (src/aes_gcm.vhd:207-211: GHASH consumes the GCTR output).
 * Copies H2D/D2H around the device path below; meant for parity tests and small messages. */
AESGCM_API int aesgcm_encrypt(aesgcm_ctx *ctx, const uint8_t iv[12], const uint8_t *aad, size_t aad_len,
                   const uint8_t *pt, size_t len, uint8_t *ct, uint8_t tag[16]);
/* Decrypt mode (tb/gcm_model.py:29-30,43-51; src/aes_gcm.vhd:207-211: GHASH consumes the input).
 * Plaintext is always written (the model emits data before the tag is checked).  tag_out (may be
 * NULL) receives the computed tag.  If expect_tag != NULL it is compared in constant time and
 * AESGCM_EAUTH is returned on mismatch. */
AESGCM_API int aesgcm_decrypt(aesgcm_ctx *ctx, const uint8_t iv[12], const uint8_t *aad, size_t aad_len,
                   const uint8_t *ct, size_t len, uint8_t *pt, const uint8_t *expect_tag, uint8_t tag_out[16]);

/* ---------------------------------------------------------------- whole messages, device pointers
 * The benchmarked path: d_in/d_out are device pointers (16-byte aligned, may alias for in-place),
 * d_aad a device pointer (any alignment) or NULL.  Work is enqueued on `stream` (a hipStream_t
 * passed as void*, NULL = context stream); the only host traffic is the 16-byte tag.  When the call
 * returns with a tag, the whole result is in device memory: the kernel that finishes the tag stores it
 * in a pinned host slot behind the data (messages of 64 KiB .. 1 GiB: the one launch that encrypts
 * the message, whose ciphertext stores go through the L2 for that), and the call returns when the
 * slot shows it -- long work falls back to a stream synchronisation.  The launch itself may retire a
 * few microseconds later; anything ordered behind it on `stream`, hipStreamSynchronize and blocking
 * copies see it complete as always.  Pass tag = NULL to skip the wait: the call only enqueues, and
 * aesgcm_last_tag() later collects the tag of the context's most recent message the same way (a poll of
 * the host slot) -- several contexts of one key, each with its own stream, keep several messages in
 * flight that way (bench.py --inflight).
 * What the call touches, in every launch structure the library may choose: it reads exactly `len`
 * bytes of d_in and `aad_len` bytes of d_aad, and writes exactly `len` bytes of d_out -- nothing in
 * front of either range and nothing behind a ragged end, so no slack up to the next 16 bytes (or row,
 * or vector store) is needed and neighbouring buffers may touch.  Out of place, d_in and d_aad are
 * left as they were.  aesgcm_decrypt_dev with expect_tag that fails verification under the context
 * option "wipe_on_auth_fail" zeroes exactly those `len` bytes of d_pt.  aesgcm_keystream_dev writes
 * exactly 16 * nblocks bytes; a refused call writes nothing.  (tests/test_gpu_msg_grid.py) */
AESGCM_API int aesgcm_encrypt_dev(aesgcm_ctx *ctx, const uint8_t iv[12], const void *d_aad, size_t aad_len,
                       const void *d_pt, size_t len, void *d_ct, uint8_t tag[16], void *stream);
AESGCM_API int aesgcm_decrypt_dev(aesgcm_ctx *ctx, const uint8_t iv[12], const void *d_aad, size_t aad_len,
                       const void *d_ct, size_t len, void *d_pt, const uint8_t *expect_tag,
                       uint8_t tag_out[16], void *stream);
/* (`stream` must be the stream the message was enqueued on: AESGCM_ESTATE if that stream has drained and the host slot still does not show the message's tag) */
AESGCM_API int aesgcm_last_tag(aesgcm_ctx *ctx, uint8_t tag[16], void *stream);

/* CTR keystream blocks [first_block, first_block+nblocks): E_K(IV || (2+i) mod 2^32)
 * (src/aes_icb.vhd:97-100,118; src/gcm_gctr.vhd:150 before the xor). */
AESGCM_API int aesgcm_keystream(aesgcm_ctx *ctx, const uint8_t iv[12], uint64_t first_block, uint64_t nblocks, uint8_t *out);
AESGCM_API int aesgcm_keystream_dev(aesgcm_ctx *ctx, const uint8_t iv[12], uint64_t first_block, uint64_t nblocks,
                         void *d_out, void *stream);

/* ---------------------------------------------------------------- one message sharded over ranks
 * (no reference counterpart: the RTL is one pipeline; the algebra is gcm_ghash.vhd:317-333's
 * linear split generalised).  Rank g owns data blocks [first_block, first_block + ceil(len/16)) of a
 * message with total_len bytes of data and aad_len bytes of AAD; only the LAST shard may have a
 * ragged length.  The rank that owns first_block == 0 also absorbs the AAD (pass d_aad there, NULL
 * elsewhere).  The call en/decrypts the shard and writes its 16-byte WEIGHTED GHASH partial
 *    W_g = (sum_{i in shard} X_i * H^(end_g-1-i)) * H^(n_total_blocks - end_g)
 * to d_partial (device memory).  Partials of all ranks are exchanged by the caller (one 16-byte
 * all-gather, e.g. RCCL) and handed to aesgcm_shard_finalize, which XOR-folds them on the device and
 * produces tag = GHASH xor E_K(IV||1).
 * A shard reads exactly `len` bytes of d_in (rank 0: and aad_len of d_aad) and writes exactly `len`
 * bytes of d_out and the 16 bytes of d_partial, from whatever first block: the ranks of one message
 * may write one buffer in any order, each leaves its neighbours' ranges alone. */
AESGCM_API int aesgcm_shard_crypt_dev(aesgcm_ctx *ctx, int decrypt, const uint8_t iv[12],
                           const void *d_aad, size_t aad_len,
                           const void *d_in, size_t len, void *d_out,
                           uint64_t first_block, uint64_t total_len,
                           void *d_partial, void *stream);
AESGCM_API int aesgcm_shard_finalize_dev(aesgcm_ctx *ctx, const uint8_t iv[12], const void *d_partials, size_t n_partials,
                              size_t aad_len, uint64_t total_len, uint8_t tag[16], void *stream);
/* The same with the n_partials partials stride_bytes apart (a multiple of 16): ONE all-gather of M messages' partials
 * leaves them as [rank][message][16]; message m is finalised from d_partials + 16 m with stride 16 M. */
AESGCM_API int aesgcm_shard_finalize_strided_dev(aesgcm_ctx *ctx, const uint8_t iv[12], const void *d_partials, size_t n_partials,
                              size_t stride_bytes, size_t aad_len, uint64_t total_len, uint8_t tag[16], void *stream);

/* The tags of n_msgs (<= 8) messages after ONE all-gather, in one launch and one wait: message m has IV ivs + 12 m, lengths
 * aad_lens[m] (NULL = all zero) / total_lens[m], its n_partials partials start at d_partials + m * msg_stride_bytes and lie
 * stride_bytes apart; tags receives n_msgs * 16 bytes.  With the [rank][message][16] layout: msg_stride_bytes = 16,
 * stride_bytes = 16 * n_msgs.  Same arithmetic as aesgcm_shard_finalize_strided_dev called n_msgs times. */
AESGCM_API int aesgcm_shard_finalize_batch_dev(aesgcm_ctx *ctx, size_t n_msgs, const uint8_t *ivs, const void *d_partials, size_t n_partials,
                              size_t stride_bytes, size_t msg_stride_bytes, const size_t *aad_lens, const uint64_t *total_lens,
                              uint8_t *tags, void *stream);

/* ---------------------------------------------------------------- the exchange step, in the library
 * (BASELINE north_star "a single RCCL reduce of per-shard partial tags over xGMI".)  RCCL has
 * no XOR reduction (rccl.h ncclRedOp_t), so the 16-byte partials are all-gathered and folded on the device by
 * aesgcm_shard_finalize_dev.  RCCL is loaded with dlopen("librccl.so.1") on first use; without it these return
 * AESGCM_ERCCL and everything else in the library still works.
 *
 * One PROCESS per GPU: rank 0 calls aesgcm_comm_unique_id and hands the 128 bytes to the other ranks by any means
 * (bench.py: a file under /tmp keyed by the launcher's pid); every rank then calls aesgcm_comm_create, which is
 * ncclCommInitRank on `device`.  aesgcm_comm_ranks returns what RCCL reports (ncclCommCount / ncclCommUserRank).
 * aesgcm_comm_allgather_dev: d_recv[r * bytes_per_rank ..] = rank r's d_send, asynchronous on `stream`.
 * aesgcm_comm_allreduce_f64: one host double, op 0 = max, 1 = min, 2 = sum, synchronous (bench timing);
 * aesgcm_comm_barrier is the sum of ones. */
#define AESGCM_COMM_ID_BYTES 128
typedef struct aesgcm_comm aesgcm_comm;
AESGCM_API const char *aesgcm_comm_last_error(void);
AESGCM_API int aesgcm_comm_unique_id(uint8_t id[AESGCM_COMM_ID_BYTES]);
AESGCM_API int aesgcm_comm_create(aesgcm_comm **out, int device, const uint8_t id[AESGCM_COMM_ID_BYTES], int n_ranks, int rank);
AESGCM_API int aesgcm_comm_ranks(const aesgcm_comm *comm, int *n_ranks, int *rank);
AESGCM_API int aesgcm_comm_allgather_dev(aesgcm_comm *comm, const void *d_send, void *d_recv, size_t bytes_per_rank, void *stream);
AESGCM_API int aesgcm_comm_allreduce_f64(aesgcm_comm *comm, double *value, int op);
AESGCM_API int aesgcm_comm_barrier(aesgcm_comm *comm);
AESGCM_API int aesgcm_comm_destroy(aesgcm_comm *comm);

/* One process driving ndev GPUs (ncclCommInitAll).  Shard g = d_in[g] / d_out[g] (device memory of devices[g]),
 * shard_len[g] bytes, owning the message's blocks right after shard g-1's; every length but the last must be a
 * multiple of 16.  Each device expands the key and builds H and its tables itself (nothing is broadcast); the AAD
 * (device memory of devices[0]) is absorbed by shard 0.  The call en/decrypts all shards concurrently, performs ONE
 * grouped ncclAllGather of 16 bytes per device, folds on devices[0] and returns the tag; all streams are
 * synchronised on return.  aesgcm_mgpu_ranks returns the communicator size RCCL reports. */
typedef struct aesgcm_mgpu aesgcm_mgpu;
AESGCM_API int aesgcm_mgpu_create(aesgcm_mgpu **out, int ndev, const int *devices, const uint8_t *key, size_t key_len);
AESGCM_API int aesgcm_mgpu_ranks(const aesgcm_mgpu *m, int *n_ranks);
AESGCM_API int aesgcm_mgpu_ctx(aesgcm_mgpu *m, int g, aesgcm_ctx **out);     /* device g's context, borrowed: never destroy it */
AESGCM_API int aesgcm_mgpu_crypt_dev(aesgcm_mgpu *m, int decrypt, const uint8_t iv[12], const void *d_aad_on_dev0, size_t aad_len,
                          const void *const *d_in, const size_t *shard_len, void *const *d_out, uint8_t tag[16]);
/* tag = NULL in aesgcm_mgpu_crypt_dev only ENQUEUES the message -- shards, the all-gather -- without a host synchronisation on any device; up to 8 such messages may
 * wait.  The queue is a FIFO: aesgcm_mgpu_last_tags finalizes the OLDEST n of them in one launch on devices[0] and returns their tags in the order they were queued (16 n bytes;
 * n may be less than what waits: the rest stays queued); aesgcm_mgpu_sync drains every device's stream (before the outputs are read by anything not ordered behind those
 * streams).  AESGCM_ESTATE when a ninth message is queued, and when a call with tag != NULL is made while messages wait (it would have to jump the queue). */
AESGCM_API int aesgcm_mgpu_last_tags(aesgcm_mgpu *m, size_t n, uint8_t *tags);
AESGCM_API int aesgcm_mgpu_sync(aesgcm_mgpu *m);
AESGCM_API int aesgcm_mgpu_destroy(aesgcm_mgpu *m);

/* ---------------------------------------------------------------- many packets under the context's key
 * The RTL keeps H across packets while no new key is loaded (src/gcm_gctr.vhd:142-144) and takes a new IV per
 * packet (src/aes_icb.vhd:60-70 "load IV"): this is that mode.  Per packet: ivs[p] (12 bytes), optional AAD
 * and data either as fixed-size records (aad_len / pkt_len, offset arrays NULL) or delimited by uint64 offset
 * arrays with n_pkts + 1 entries (then aad_len / pkt_len are ignored); tags[p] receives the computed tag; for
 * decrypt d_auth[p] (optional) = 1 if it equals d_expect_tags[p].  Asynchronous on `stream`.
 * Two families of kernels do the work.  Packets of message size -- from 8 KiB each (context option "rows_min"; from 2 KiB unless there are many between the two), up to
 * 2^28 - 1 bytes -- go BY ROWS (round 5): the 64-block rows of all such messages are one pool of work for the row loop a single large message runs through
 * (csrc/aesgcm_rows.h), and one small launch behind it takes what is not a whole row -- headers, ragged ends -- block by block and closes every tag; 4096 x 1 MiB then runs
 * at the rate of one 4 GiB message.  Shorter packets take the packet kernels: a lane, or a group of 4 .. 16 lanes, per packet.
 * FIXED-SIZE records: the host knows the one size and the whole call goes one way (many records of 8 .. 16 KiB whose last partial row is longer than 4 blocks stay with the
 * packet kernels).  OFFSET ARRAYS: the lengths are on the device, and so is the choice -- every message is ROUTED BY ITS OWN SIZE (data + AAD) inside the one call (round 6):
 * a counting sort by size class on the device (three small launches on `stream`) splits the call at the mark, hands the short messages to the packet kernels longest first
 * (the lanes of a wave run to the longest packet among them) and the others to the rows; which path a message takes never shows in its bytes or its tag.  The reference's
 * own traffic is of both kinds at once (tb/gcm_gctr.py:279-281: lengths from a U-shaped distribution).  pkt_len is IGNORED with offset arrays (until round 5 it was a hint
 * that sent the whole call one way).  Lengths of 2^28 bytes or more, or offsets that do not rise, are found on the device: nothing of the call runs then, see aesgcm_ctx_status.
 * CAPTURE: for given pointers and count the host's side of a routed call is a fixed sequence of launches on `stream` and the context's side stream (forked and joined by
 * events).  After one ordinary call of the same context with sizes at least as large, this call and aesgcm_messages_crypt_dev allocate nothing, wait for nothing and read
 * nothing back, so they may run under hipStreamBeginCapture on `stream`; the graph may be replayed over other lengths, offsets and bytes (examples/graph_replay.cpp,
 * tests/test_gpu_mixed.py; on ROCm 7.2 a replay costs what the direct call costs). */
AESGCM_API int aesgcm_packets_crypt_dev(aesgcm_ctx *ctx, int decrypt, size_t n_pkts, const void *d_ivs,
                             const void *d_aad, size_t aad_len, const uint64_t *d_aad_off,
                             const void *d_in, size_t pkt_len, const uint64_t *d_data_off, void *d_out,
                             void *d_tags, const void *d_expect_tags, int *d_auth, void *stream);

/* Messages WHEREVER THEY LIVE under the context's key (round 5): the same work as aesgcm_packets_crypt_dev with offset arrays, but every message has its own buffers --
 * the reference's harness hands the core one frame after the other, each its own object (tb/gcm_test.py:76-85, tb/gcm_gctr.py:233-276); a caller with a queue
 * of messages in separate allocations has exactly that, and copying them into one buffer to batch them would cost what the batch saves.  All arrays are in
 * device memory, n_msgs entries each: d_in_ptr / d_out_ptr device addresses of the messages' input and output (in == out allowed), d_len their lengths
 * (each < 2^28 bytes), d_aad_ptr / d_aad_len the same for AAD (both NULL: none); d_ivs n_msgs x 12 bytes, d_tags n_msgs x 16; decrypt: d_expect_tags / d_auth
 * as aesgcm_packets_crypt_dev.  Routed per message like the offset-array form (round 6: until then always by rows, and a call of tiny messages paid for it); the
 * context option "wipe_on_auth_fail" applies; a length of 2^28 or more is reported through aesgcm_ctx_status.  Asynchronous on `stream`. */
AESGCM_API int aesgcm_messages_crypt_dev(aesgcm_ctx *ctx, int decrypt, size_t n_msgs, const void *d_ivs,
                              const uint64_t *d_aad_ptr, const uint32_t *d_aad_len,
                              const uint64_t *d_in_ptr, const uint32_t *d_len, const uint64_t *d_out_ptr,
                              void *d_tags, const void *d_expect_tags, int *d_auth, void *stream);

/* ---------------------------------------------------------------- batch: independent packets, per-packet key + IV
 * (BASELINE config 5; the RTL equivalent is reloading key and IV between packets, tb/gcm_gctr.py:144-175,
 * with aes_kexp run per packet, config/config_aes_kexp.py:113-159.)  All arrays are contiguous device memory:
 * keys[n][key_len], ivs[n][12], aad[n][aad_len] (or NULL), in[n][pkt_len], out[n][pkt_len], tags[n][16].
 * One wave per packet; key expansion, H, E_K(J0) and the GHASH tables are rebuilt per packet on the GPU.
 * decrypt != 0: GHASH runs over the input, tags[] receives the COMPUTED tags; if d_auth != NULL it receives
 * one int per packet (1 = equals d_expect_tags[p], 0 = mismatch; all 1 when d_expect_tags is NULL).
 * Asynchronous on `stream`; in == out is allowed. */
AESGCM_API int aesgcm_batch_crypt_dev(int device, int decrypt, size_t n_pkts, size_t key_len, const void *d_keys, const void *d_ivs,
                           const void *d_aad, size_t aad_len, const void *d_in, size_t pkt_len, void *d_out,
                           void *d_tags, const void *d_expect_tags, int *d_auth, void *stream);

/* Zero the output of every packet whose d_auth entry is 0: what the context option "wipe_on_auth_fail" does behind aesgcm_packets_crypt_dev, for callers of the
 * context-free batch entry points (fixed-size records: d_data_off = NULL).  Asynchronous on `stream`, which must be the stream the decrypt call ran on.
 * Bound: a packet whose range falls (d_data_off[p + 1] < d_data_off[p]) or is 2^28 bytes or more long -- a length no call of this library accepts -- is left
 * untouched, whatever its d_auth entry says; so is every packet behind a context call that was refused (aesgcm_ctx_status). */
AESGCM_API int aesgcm_wipe_failed_dev(int device, size_t n_pkts, void *d_out, size_t pkt_len, const uint64_t *d_data_off, const int *d_auth, void *stream);

/* Measurement support: the batch kernel's instruction stream without the data's loads and stores (keys, IVs and tags still move) over n_pkts virtual packets of
 * pkt_len bytes -- the ceiling of its formulation (per-packet aes_kexp, T-table AES, Shoup GHASH) on this chip at this moment's clocks; the caller times it
 * (aesgcm_timer_*).  Only for calls that take the 8-lanes-per-packet shape, as BASELINE config 5 does (AESGCM_EARG otherwise). */
AESGCM_API int aesgcm_batch_ceiling_probe_dev(int device, size_t n_pkts, size_t key_len, const void *d_keys, const void *d_ivs, size_t pkt_len, void *d_tags, void *stream);

/* The same for the frame path (round 6): the packet kernels' instruction stream over n_pkts frames delimited by d_data_off (and d_aad_off: or NULL) as aesgcm_packets_crypt_dev
 * takes them, WITHOUT the data's loads and stores (IVs, offsets, AAD and tags still move; no data buffer is passed) -- every frame to the packet kernels, in the shape the
 * device chooses for the count.  bench.py --config frames prints it as roofline.formulation_ceiling.  Asynchronous on `stream`; the caller times it. */
AESGCM_API int aesgcm_frames_ceiling_probe_dev(aesgcm_ctx *ctx, size_t n_pkts, const void *d_ivs, const void *d_aad, const uint64_t *d_aad_off, const uint64_t *d_data_off, void *d_tags, void *stream);

/* Which kernel shape a call with these arguments takes: lanes per packet (1 = one lane per packet, 4 / 8 / 16 = a lane group, 64 = a
 * whole wave; aesgcm_packets_shape: AESGCM_SHAPE_ROWS = by rows, every message over the whole chip).  var_len != 0 describes the offset-array forms:
 * aesgcm_batch_shape goes by count (the host does not know the lengths); aesgcm_packets_shape answers AESGCM_SHAPE_MIXED -- every message is routed by
 * its own size on the device, by rows or to the packet kernel shape chosen there for the count of short ones (pkt_len is ignored). */
#define AESGCM_SHAPE_ROWS (1 << 20)
#define AESGCM_SHAPE_MIXED (1 << 21)
/* ... and what the device DID decide for the context's most recent call of that kind (waits for the device): out[0] = the mark in bytes -- messages of at least that size
 * (data + AAD) went by rows; 0 = all of them, 0xFFFFFFFF = none --, out[1] = messages that took the packet kernels, out[2] = lanes per packet of the packet kernel shape
 * chosen for that count (0: no packet launch did anything), out[3] = units (rows, long tails, long AADs) of the row launch.  AESGCM_ESTATE before the first such call. */
AESGCM_API int aesgcm_ctx_last_route(aesgcm_ctx *ctx, uint64_t out[4]);
AESGCM_API int aesgcm_batch_shape(int device, size_t n_pkts, size_t pkt_len, int var_len, int *lanes_per_packet);
AESGCM_API int aesgcm_packets_shape(const aesgcm_ctx *ctx, size_t n_pkts, size_t pkt_len, int var_len, int *lanes_per_packet);

/* Variable-length form (MACsec-shaped traffic like the reference's README vectors: short frames with a
 * per-frame header as AAD, README.md:251-257): packet p occupies bytes [d_data_off[p], d_data_off[p+1]) of
 * in/out and, when d_aad_off != NULL, bytes [d_aad_off[p], d_aad_off[p+1]) of aad.  Offset arrays have
 * n_pkts + 1 uint64 entries in device memory.  Each packet < 2^28 bytes, and offsets must rise: the caller's to ensure -- unlike the context's offset-array calls,
 * this entry point does NOT check the lengths on the device (nothing refuses a call with a longer packet or falling offsets).  Packets whose data offset is a
 * multiple of 16 take the aligned fast path.  From 262144 packets (AES-128; 98304 for the longer keys) the launch takes them by falling
 * length class, as aesgcm_packets_crypt_dev does (scratch: 4 bytes per packet, kept per device). */
AESGCM_API int aesgcm_batch_crypt_var_dev(int device, int decrypt, size_t n_pkts, size_t key_len, const void *d_keys, const void *d_ivs,
                               const void *d_aad, const uint64_t *d_aad_off, const void *d_in, const uint64_t *d_data_off,
                               void *d_out, void *d_tags, const void *d_expect_tags, int *d_auth, void *stream);

/* ---------------------------------------------------------------- key tables: batches of many keys without per-packet key setup
 * Between one key per context and one raw key per packet (the batch entry points above): a MACsec SecY with many secure associations, an IPsec gateway, a TLS
 * terminator -- thousands of keys, each used for many packets and changed rarely; the reference's own pre-expanded-key mode (config/config_aes_kprexp.py) and its
 * harness, which loads a key and then sends frame after frame under it (tb/gcm_gctr.py:144-175).  A table is device memory of n_slots slots of ONE key size
 * (16, 24 or 32 bytes); a slot holds the round keys, H and the powers H^(2^j) of the GHASH Horner strides, computed on the GPU once when the key is set -- none of
 * it is ever copied back to the host, and there is no call to read it.  A crypt call names a slot per packet and runs the batch kernel's loop without the
 * per-packet key schedule, H = E_K(0) and squaring chain; E_K(J0) stays per packet.
 *   aesgcm_keytab_create   n_slots zeroed slots, all unset (n_slots < 2^31).  AESGCM_EHIP without a usable device.
 *   aesgcm_keytab_set      keys[n][key_len] from HOST memory into slots first_slot .. first_slot + n - 1 (AESGCM_EARG past the end).  The keys pass through a
 *                          device staging buffer of the table that is zeroed on `stream` as soon as the expansion has read it; `keys` may be reused on return.
 *   aesgcm_keytab_set_dev  d_keys[n][key_len] in DEVICE memory into the slots d_slots[0 .. n-1] (device memory).  An entry whose slot is n_slots or more is skipped and
 *                          reported through aesgcm_keytab_status (detail = its index in d_slots); a slot named twice in one call takes one of its keys.
 *   aesgcm_keytab_clear    retire slots first_slot .. first_slot + n - 1: zeroed and unset; packets that name them are refused from then on.
 *   aesgcm_keytab_crypt_dev  n_pkts packets, packet p under slot d_slots[p]; the other arguments as aesgcm_packets_crypt_dev: fixed-size records (d_aad_off and
 *                          d_data_off NULL: aad_len / pkt_len bytes each, < 2^28, packets back to back) or offset arrays of n_pkts + 1 uint64 entries (aad_len /
 *                          pkt_len then ignored; d_aad_off NULL = no AAD).  d_ivs[n][12], d_tags[n][16] (decrypt: the COMPUTED tags), d_auth[p] (decrypt, optional)
 *                          = 1 if the tag equals d_expect_tags[p] (all 1 when that is NULL).  Shape and order as aesgcm_batch_crypt_var_dev: 8, 16 or 64 lanes per
 *                          packet by count (aesgcm_batch_shape), by falling length class from 262144 packets (98304 for the longer keys).  A long packet still runs
 *                          on one lane group: key tables do not route messages of megabytes to the row kernels (use a context for those).
 *   A packet the device cannot process -- its slot is n_slots or more, unset or cleared; its data or AAD range falls (an offset below the one before) or is 2^28
 *   bytes or more -- is REFUSED on its own: its output bytes are left untouched (nothing else of it is read), its tag is written as 16 zero bytes, d_auth[p] = 0 on
 *   decrypt, and the table's status word records it.  Every other packet of the call is processed normally; an out-of-range slot is never read.
 *   aesgcm_keytab_status   *code = AESGCM_EARG and *detail = the LOWEST refused packet (or skipped set_dev entry) since the last read, or AESGCM_OK and 0.  Reading
 *                          clears it.  It does not wait for calls in flight: synchronise the streams they ran on first.
 *   aesgcm_keytab_destroy  waits for the device, zeroes the slots and the staging buffer, frees them.
 * Decrypt outputs work with aesgcm_wipe_failed_dev (a refused packet has d_auth = 0; a falling or too-long range is left untouched by it as well).
 * ORDERING: every call is asynchronous and stream-ordered on `stream` (NULL = the null stream).  A set or clear on stream A and a crypt call on stream B that names
 * the same slot are NOT ordered by the library: the caller orders them (an event, or one stream for both).  Key rotation: set the new key into an unused slot,
 * switch the packets' slot numbers to it, clear the old slot once no call in flight names it (INTEGRATION.md "Key tables").  The calls of one table are
 * thread-safe; a table belongs to the device it was created on.
 * CAPTURE (key tables and receive windows): every aesgcm_keytab_*_crypt_dev call, aesgcm_rxwin_recover_dev, aesgcm_rxwin_commit_dev, aesgcm_txnum_assign_dev and aesgcm_wipe_failed_dev is a
 * fixed sequence of launches (and one 4-byte memset node per crypt call) on `stream` for given pointers and counts: no allocation, no host synchronisation, nothing read
 * back, no event.  They may run under hipStreamBeginCapture on `stream` (a created stream; thread-local capture mode suffices), several of them behind one another, and
 * the graph may be replayed over other slots, numbers, lengths, offsets and bytes in the same buffers; a receive loop's window state travels from replay to replay in
 * the window records.  (The five-array aesgcm_batch_crypt_dev / _var_dev plan their launch the same way and follow the same rules.)
 * aesgcm_kdf_install_dev and aesgcm_kdf_update_dev ("ON-DEVICE KEY DERIVATION" below) belong to this list too: one launch each, no memset node, no dispenser; the
 * graph holds the secret records beside the slots, and a replayed update in place steps its secrets one generation per replay.  So does aesgcm_srtp_kdf_install_dev
 * ("SRTP KEY DERIVATION" below): one launch, and the graph holds the master records beside the slots.  So do aesgcm_prf12_install_dev and aesgcm_prf12_export_srtp_dev
 * ("TLS 1.2 PRF" below): one launch each, and the graph holds the master-secret records beside the slots (install) or beside the SRTP master records (export).  So does
 * aesgcm_prfplus_install_dev ("IKEv2 PRF+" below): one launch, and the graph holds the SK_d records and the caller's seed buffer and offsets beside the slots.
 * So do aesgcm_mka_install_dev and aesgcm_mka_unwrap_dev ("MACSEC MKA" below): one launch each, and the graph holds the CAK records and the caller's context buffer and
 * offsets, wrapped-key buffer and verdict bytes beside the slots.  So does aesgcm_sshkdf_install_dev ("SSH KEY DERIVATION" below): one launch, and the graph holds
 * the secret records beside the slots.
 *   PRECONDITION     one ordinary call on that device, with that table (or window table) and key size, before the capture: per-device state is made on first use.
 *   A GRAPH HOLDS    the caller's pointers and n, the table's slots and status word, the window records, the counter records and the counter table's scratch, and ONE of the device's 256 launch dispensers (a word the
 *                    lane groups draw packets from, zeroed by the graph's memset node).  Destroy the graph before the table; the caller's buffers are the caller's.
 *   ORDERING         a captured call is never ordered by falling length class, whatever its count: the order's scratch belongs to the device, not to the graph.  The
 *                    packets are taken in array order -- the same bytes, slower from the counts at which an ordinary call is ordered.
 *   NOT CAPTURE-SAFE aesgcm_keytab_create, every aesgcm_keytab_set*, aesgcm_keytab_status, _destroy; aesgcm_rxwin_create, _set, _get, _status, _destroy; aesgcm_txnum_create, _set, _get, _status, _destroy (staging buffers
 *                    that grow, events, synchronous copies, waits): call them outside the capture.  So are aesgcm_kdf_create, _set, _set_dev, _clear, _status, _destroy
 *                    and aesgcm_srtp_kdf_create, _set, _set_dev, _clear, _status, _destroy, and aesgcm_prf12_create, _set, _set_dev, _clear, _status, _destroy,
 *                    and aesgcm_prfplus_create, _set, _set_dev, _clear, _status, _destroy, and aesgcm_mka_create, _set, _set_dev, _clear, _status, _destroy,
 *                    and aesgcm_sshkdf_create, _set, _set_dev, _clear, _status, _destroy.
 *   DISPENSERS       a replay shares its dispenser with every 256th later crypt call on the device.  On one stream that is harmless (each zeroes it before use).
 *                    Such a call must not run CONCURRENTLY with the replay on another stream: a caller who replays graphs beside ordinary calls on other streams
 *                    orders them, or keeps fewer than 256 crypt calls between a graph's capture and its last replay.
 * tests/test_gpu_capture.py replays every family against libcrypto; tests/fake_hip/capture_drive.py holds the host side to the list above. */
typedef struct aesgcm_keytab aesgcm_keytab;
AESGCM_API int aesgcm_keytab_create(aesgcm_keytab **out, int device, size_t key_len, size_t n_slots);
AESGCM_API int aesgcm_keytab_set(aesgcm_keytab *t, size_t first_slot, size_t n, const uint8_t *keys, void *stream);
AESGCM_API int aesgcm_keytab_set_dev(aesgcm_keytab *t, size_t n, const uint32_t *d_slots, const void *d_keys, void *stream);
AESGCM_API int aesgcm_keytab_clear(aesgcm_keytab *t, size_t first_slot, size_t n, void *stream);
AESGCM_API int aesgcm_keytab_crypt_dev(aesgcm_keytab *t, int decrypt, size_t n_pkts, const uint32_t *d_slots, const void *d_ivs,
                            const void *d_aad, size_t aad_len, const uint64_t *d_aad_off,
                            const void *d_in, size_t pkt_len, const uint64_t *d_data_off, void *d_out,
                            void *d_tags, const void *d_expect_tags, int *d_auth, void *stream);
AESGCM_API int aesgcm_keytab_status(aesgcm_keytab *t, int *code, uint64_t *detail);
AESGCM_API int aesgcm_keytab_destroy(aesgcm_keytab *t);

/* ---------------------------------------------------------------- key tables on frames in WIRE FORMAT (MACsec, ESP): one buffer, one launch
 * What a SecY or an IPsec gateway holds is not five parallel arrays but FRAMES: one byte-packed buffer in which every frame is header | payload | ICV, the nonce partly
 * in the header and partly a constant of the secure association, the ICV 8, 12 or 16 bytes.  aesgcm_keytab_frames_crypt_dev takes that buffer as it is: frame p is bytes
 * [d_frame_off[p], d_frame_off[p + 1]) of d_in and of d_out (the same n_frames + 1 offsets for both; d_in == d_out allowed; any byte alignment), laid out by *fmt, which
 * is per call:
 *   bytes [0, aad_len)              authenticated, pass through unchanged
 *   bytes [aad_len, hdr_len)        pass through, NOT authenticated (ESP's explicit IV field)
 *   bytes [hdr_len, len - tag_len)  the payload: encrypted / decrypted (length 0 is legal)
 *   the last tag_len bytes          the ICV = the leading tag_len bytes of the GCM tag
 *   nonce                           salt[0 .. salt_len) of the frame's slot, then the 12 - salt_len frame bytes at iv_off (which end at hdr_len at the latest)
 * The SALT is 8 bytes of slot state beside the key material: zero after aesgcm_keytab_create and aesgcm_keytab_clear, left alone by aesgcm_keytab_set / _set_dev,
 * written by aesgcm_keytab_set_salt (salts[n][8] in HOST memory into slots first_slot .. first_slot + n - 1; stream-ordered like aesgcm_keytab_set; a format with
 * salt_len 4 uses the first four bytes).
 * Encrypt: the payload is encrypted and the ICV written.  Decrypt: the payload is decrypted and d_auth[p] = 1 iff the ICV in d_in equals the leading tag_len bytes of
 * the computed tag (d_auth is required for decrypt and ignored for encrypt).  Out of place every byte of an accepted frame in d_out is defined: the header is copied,
 * and on decrypt the ICV.  No byte outside an accepted frame's range and no byte at all of a refused frame is written.
 * AESGCM_WIRE_AUTH_ONLY: nothing is encrypted; every byte in front of the ICV is AAD (MACsec integrity-only, E = 0; GMAC) and passes through.
 * A frame the device cannot take is REFUSED on its own, as aesgcm_keytab_crypt_dev refuses a packet: its slot is n_slots or more, unset or cleared; its offsets fall;
 * it is 2^28 bytes or more; it is shorter than hdr_len + tag_len (auth-only: than max(hdr_len, iv_off + 12 - salt_len) + tag_len).  Its output is untouched,
 * d_auth[p] = 0 on decrypt, and the LOWEST such index goes to aesgcm_keytab_status.
 * aesgcm_wire_fmt_check: AESGCM_OK, or AESGCM_EARG for a format the call refuses as a whole -- NULL, salt_len not 0 / 4 / 8, tag_len not 8 / 12 / 16, hdr_len < aad_len
 * (unless auth-only), nonce bytes past hdr_len, an unknown flag, hdr_len >= 2^16.  It touches no device; aesgcm_keytab_frames_crypt_dev runs it first.
 * FAIL-CLOSED needs nothing new: aesgcm_wipe_failed_dev(device, n_frames, d_out, 0, d_frame_off, d_auth, stream) behind a decrypt zeroes the failed frames whole.
 * One k_kt_wire launch per call and one pass over the frame bytes; shape and order as aesgcm_keytab_crypt_dev with offset arrays (8, 16 or 64 lanes per frame by count,
 * by falling frame length class from 262144 frames, 98304 for the longer keys).  Ordering and thread safety as the other key-table calls.
 * Formats {aad_len, hdr_len, iv_off, salt_len, tag_len, flags}:
 *   MACsec, explicit SCI    {28, 28, 16, 8, 16, 0}   DA SA | SecTAG with SCI; the slot's salt = the secure channel's SCI, the PN is read at bytes 16 .. 19
 *   MACsec, no SCI          {20, 20, 16, 8, 16, 0}   the salt as above (the SCI is implicit)
 *   MACsec integrity-only   the same with AESGCM_WIRE_AUTH_ONLY (the user data is AAD as well)
 *   ESP, RFC 4106           {8, 16, 8, 4, 16 | 12 | 8, 0}   SPI, sequence number | 8-byte IV field | payload | ICV; the slot's salt = the SA's 4-byte salt
 *   MACsec confidentiality offset 30 / 50   {28 + 30, 28 + 30, 16, 8, 16, 0}: the offset's bytes are authenticated header
 * MACsec XPN and ESP with extended sequence numbers need a number that is not in the frame: aesgcm_keytab_frames_crypt_x_dev, below.
 * OUT OF SCOPE: generating packet numbers / sequence numbers (not this call's: aesgcm_txnum_assign_dev, "SEND COUNTERS" below, hands them out and writes them into the frames), anti-replay windows (not this call's: aesgcm_rxwin_*, "RECEIVE WINDOWS" below), and routing long frames to the row kernels (a frame runs on one lane
 * group).  TLS records (their AAD is not a span of the wire bytes) are not a format of this call: aesgcm_keytab_records_crypt_dev, further below. */
#define AESGCM_WIRE_AUTH_ONLY 1u   /* nothing is encrypted: every byte in front of the ICV is AAD (MACsec integrity-only, E = 0; GMAC) */
typedef struct aesgcm_wire_fmt {
    uint32_t aad_len;   /* frame bytes [0, aad_len) are authenticated and pass through unchanged                          */
    uint32_t hdr_len;   /* payload starts here; hdr_len >= aad_len; bytes [aad_len, hdr_len) pass through, unauthenticated */
    uint32_t iv_off;    /* the nonce's last 12 - salt_len bytes are frame bytes [iv_off, iv_off + 12 - salt_len) <= hdr_len */
    uint32_t salt_len;  /* 0, 4 or 8: the nonce's first bytes come from the slot's salt                                   */
    uint32_t tag_len;   /* 8, 12 or 16: the ICV = the frame's last tag_len bytes = the leading bytes of the GCM tag       */
    uint32_t flags;     /* 0 or AESGCM_WIRE_AUTH_ONLY (then aad_len is ignored; hdr_len only bounds iv_off)               */
} aesgcm_wire_fmt;
AESGCM_API int aesgcm_wire_fmt_check(const aesgcm_wire_fmt *fmt);
AESGCM_API int aesgcm_keytab_set_salt(aesgcm_keytab *t, size_t first_slot, size_t n, const uint8_t *salts, void *stream);
AESGCM_API int aesgcm_keytab_frames_crypt_dev(aesgcm_keytab *t, int decrypt, const aesgcm_wire_fmt *fmt, size_t n_frames,
                                   const uint32_t *d_slots, const void *d_in, const uint64_t *d_frame_off,
                                   void *d_out, int *d_auth, void *stream);

/* ---------------------------------------------------------------- wire frames with 64-BIT NUMBERS: MACsec XPN (IEEE 802.1AEbw), ESP with ESN (RFC 4303, RFC 4106 section 5)
 * At this library's frame rates a 32-bit packet number lasts seconds.  Both standards answer with a 64-bit number of which only the LOWER half is in the frame; the upper
 * half enters the nonce (XPN) or the AAD (ESN).  aesgcm_keytab_frames_crypt_x_dev is aesgcm_keytab_frames_crypt_dev with that half as one more array: d_hi, DEVICE memory,
 * n_frames numeric 32-bit values indexed by frame like d_slots.  A transmitter's d_hi[p] is pn >> 32 of the number it assigned; a receiver recovers it from its replay
 * window before the call (802.1AEbw 10.6.2, RFC 4303 Appendix A: aesgcm_rxwin_recover_dev with AESGCM_RXWIN_LOWEST writes exactly this array).  The format is aesgcm_wire_xfmt = a base format f and ext:
 *   ext 0                 d_hi is ignored (NULL allowed); the call IS aesgcm_keytab_frames_crypt_dev with f
 *   AESGCM_WIREX_XPN      f a MACsec format {28 | 20, 28 | 20, 16, 8, 16, 0 | AESGCM_WIRE_AUTH_ONLY} (salt_len must be 8).  Everything about the frame is as f says but the
 *                         nonce = xsalt[0..12) XOR (ssci[0..4) | be32(d_hi[p]) | frame[iv_off, iv_off + 4)): the SSCI XORs the salt's first four bytes, the 64-bit PN, big-endian,
 *                         its last eight.  xsalt and ssci are 16 bytes of slot state APART from the 8-byte salt of aesgcm_keytab_set_salt: zero after aesgcm_keytab_create and
 *                         aesgcm_keytab_clear, left alone by aesgcm_keytab_set / _set_dev / _set_salt, written by aesgcm_keytab_set_xpn (salts[n][12] and sscis[n][4] in HOST
 *                         memory, both required, into slots first_slot .. first_slot + n - 1; stream-ordered like aesgcm_keytab_set_salt).  XPN calls ignore the 8-byte
 *                         salt; calls without XPN ignore this state.
 *   AESGCM_WIREX_ESN      f an ESP format {8, 16, 8, 4, 16 | 12 | 8, 0} (aad_len must be 8, AESGCM_WIRE_AUTH_ONLY clear).  AAD = frame[0, 4) | be32(d_hi[p]) | frame[4, 8): SPI,
 *                         seq-hi, seq-lo, 12 bytes.  The nonce (the slot's 4-byte salt, the IV field), the pass-through header and the payload are as f says.
 * aesgcm_wire_xfmt_check: aesgcm_wire_fmt_check on f, then AESGCM_EARG for NULL, reserved != 0, an unknown bit in ext or both bits, XPN unless f.salt_len == 8, ESN unless
 * f.aad_len == 8 without AESGCM_WIRE_AUTH_ONLY.  It touches no device; the crypt call runs it first, and with ext != 0 it returns AESGCM_EARG for d_hi == NULL.
 * Refusals, aesgcm_keytab_status, out-of-place copies, d_auth, aesgcm_wipe_failed_dev, shape, order and thread safety are aesgcm_keytab_frames_crypt_dev's; a refused
 * frame's d_hi is not read.  One k_kt_wirex launch per call (ext 0: one k_kt_wire launch).
 * TLS 1.3 records (their nonce takes a 64-bit number with no wire part) are not a mode of this call either: d_hi holds 32-bit values.  They have a call of their own,
 * aesgcm_keytab_records_crypt_dev, below.
 * OUT OF SCOPE: recovering d_hi from a replay window, anti-replay itself (neither is this call's: aesgcm_rxwin_recover_dev / _commit_dev, "RECEIVE WINDOWS" below), generating packet numbers, writing the PN into the SecTAG (neither is this call's: aesgcm_txnum_assign_dev, "SEND COUNTERS" below, writes d_hi and the SecTAG's / the ESP header's lower half), ESN with AESGCM_WIRE_AUTH_ONLY (RFC 4543), routing long frames to the row kernels. */
#define AESGCM_WIREX_XPN 1u   /* nonce = the slot's 12-byte XPN salt XOR (the slot's SSCI | be32(d_hi[p]) | the 4 frame bytes at iv_off) */
#define AESGCM_WIREX_ESN 2u   /* AAD = frame[0,4) | be32(d_hi[p]) | frame[4,8): 12 bytes; nonce as the base format says */
typedef struct aesgcm_wire_xfmt {
    aesgcm_wire_fmt f;  /* the frame's layout, as aesgcm_keytab_frames_crypt_dev takes it */
    uint32_t ext;       /* 0, AESGCM_WIREX_XPN or AESGCM_WIREX_ESN                         */
    uint32_t reserved;  /* 0                                                              */
} aesgcm_wire_xfmt;     /* 32 bytes */
AESGCM_API int aesgcm_wire_xfmt_check(const aesgcm_wire_xfmt *xf);
AESGCM_API int aesgcm_keytab_set_xpn(aesgcm_keytab *t, size_t first_slot, size_t n, const uint8_t *salts, const uint8_t *sscis, void *stream);
AESGCM_API int aesgcm_keytab_frames_crypt_x_dev(aesgcm_keytab *t, int decrypt, const aesgcm_wire_xfmt *xf, size_t n_frames, const uint32_t *d_slots,
                                     const uint32_t *d_hi, const void *d_in, const uint64_t *d_frame_off, void *d_out, int *d_auth, void *stream);

/* ---------------------------------------------------------------- key tables on TLS RECORDS in wire format: TLS 1.3 (RFC 8446) and TLS 1.2 AES-GCM (RFC 5288)
 * What a TLS terminator holds is one buffer of records header | ciphertext | tag.  Neither call above can express one: a TLS 1.3 nonce takes the record's 64-bit sequence
 * number, of which no byte is on the wire, and a TLS 1.2 AAD is not a span of the record's bytes.  aesgcm_keytab_records_crypt_dev takes the buffer as it is: record p is
 * bytes [d_rec_off[p], d_rec_off[p + 1]) of d_in and of d_out (the same n_recs + 1 offsets for both; d_in == d_out allowed; any byte alignment), L bytes long, under slot
 * d_slots[p], with the sequence number d_seq[p]: DEVICE memory, n_recs numeric 64-bit values (the kernel forms their big-endian bytes).  fmt->version says which record:
 *   AESGCM_TLS_13   hdr[5] | payload | tag[16]  (RFC 8446 5.2, 5.3).  AAD = the five header bytes as they lie in the buffer.  Nonce = the slot's 12-byte IV XOR
 *                   (00 00 00 00 | be64(d_seq[p])).  The payload (TLSInnerPlaintext: content, content type, padding) is not interpreted; length 0 is taken.  L >= 21.
 *   AESGCM_TLS_12   hdr[5] | explicit_nonce[8] | payload | tag[16]  (RFC 5288 3, RFC 5246 6.2.3.3).  Nonce = the slot IV's first four bytes, then the record's eight
 *                   explicit bytes.  AAD = be64(d_seq[p]) | hdr[0..3) | be16(L - 29), 13 bytes: type and version from the record, the LENGTH FROM THE OFFSETS -- the
 *                   header's own two length bytes are not read for it.  Header and explicit nonce pass through.  L >= 29.
 * The slot's IV is 12 bytes of slot state: the client_write_iv / server_write_iv of the connection direction the slot stands for (TLS 1.2: its four bytes, the rest
 * ignored), written by aesgcm_keytab_set_tls_iv (ivs[n][12] in HOST memory into slots first_slot .. first_slot + n - 1; stream-ordered like aesgcm_keytab_set_xpn, through the
 * zeroed staging buffer).  It lies in the 16 bytes that hold MACsec XPN's salt and SSCI: a slot is a MACsec association or a TLS connection direction, never both, and
 * aesgcm_keytab_set_xpn and aesgcm_keytab_set_tls_iv OVERWRITE one another (set_tls_iv leaves the SSCI's place zero).  Zero after aesgcm_keytab_create and
 * aesgcm_keytab_clear, left alone by aesgcm_keytab_set / _set_dev / _set_salt.
 * Encrypt writes the payload and the tag; the caller wrote the header and, for 1.2, the explicit nonce, as a SecY writes its SecTAG.  Decrypt writes the payload and
 * d_auth[p] = 1 iff the record's tag equals the computed one (d_auth is required for decrypt and ignored for encrypt).  Out of place every byte of an accepted record in
 * d_out is defined: the header (1.2: and the explicit nonce) is copied, and on decrypt the tag.  No byte outside an accepted record is written.
 * A record the device cannot take is REFUSED on its own, exactly as aesgcm_keytab_frames_crypt_dev refuses a frame: its slot is n_slots or more, unset or cleared; its
 * offsets fall; L is below the shortest record; L - 5 > 65535 (the wire's length field cannot say it).  Nothing of it is written, d_seq[p] is not read, d_auth[p] = 0 on
 * decrypt, and the LOWEST such index goes to aesgcm_keytab_status.  FAIL-CLOSED: aesgcm_wipe_failed_dev(device, n_recs, d_out, 0, d_rec_off, d_auth, stream) behind a decrypt.
 * aesgcm_tls_fmt_check: AESGCM_EARG for NULL, a version other than AESGCM_TLS_13 / AESGCM_TLS_12, reserved != 0.  It touches no device; the crypt call runs it first,
 * then returns AESGCM_EARG for d_seq == NULL, both before it looks at the table.
 * One k_kt_tls launch per call; shape and order as aesgcm_keytab_frames_crypt_dev (8, 16 or 64 lanes per record by count, by falling length class from 262144 records, 98304
 * for the longer keys).  Ordering and thread safety as the other key-table calls.
 * OUT OF SCOPE: checking the header's version, type or length bytes against the offsets; padding and content type (the payload's last bytes in 1.3); generating sequence
 * numbers or explicit nonces (not this call's: aesgcm_txnum_assign_dev, "SEND COUNTERS" below, gives d_seq and writes 1.2's explicit nonce); key derivation (INTEGRATION.md "TLS records" says which secret becomes what); routing long records to the row kernels.  (DTLS records: aesgcm_keytab_dtls_crypt_dev below.) */
#define AESGCM_TLS_13 1u   /* hdr[5] | payload | tag[16]; nonce = slot IV XOR (0^32 | be64(d_seq[p])); AAD = hdr */
#define AESGCM_TLS_12 2u   /* hdr[5] | explicit nonce[8] | payload | tag[16]; nonce = slot IV[0..4) | explicit nonce; AAD = be64(d_seq[p]) | hdr[0..3) | be16(L - 29) */
typedef struct aesgcm_tls_fmt {
    uint32_t version;   /* AESGCM_TLS_13 or AESGCM_TLS_12 */
    uint32_t reserved;  /* 0                              */
} aesgcm_tls_fmt;       /* 8 bytes */
AESGCM_API int aesgcm_tls_fmt_check(const aesgcm_tls_fmt *fmt);
AESGCM_API int aesgcm_keytab_set_tls_iv(aesgcm_keytab *t, size_t first_slot, size_t n, const uint8_t *ivs, void *stream);
AESGCM_API int aesgcm_keytab_records_crypt_dev(aesgcm_keytab *t, int decrypt, const aesgcm_tls_fmt *fmt, size_t n_recs, const uint32_t *d_slots, const uint64_t *d_seq,
                                    const void *d_in, const uint64_t *d_rec_off, void *d_out, int *d_auth, void *stream);

/* ---------------------------------------------------------------- key tables on QUIC PACKETS in wire format, with header protection (RFC 9001 section 5, AES-GCM suites)
 * What an HTTP/3 terminator holds is one buffer of QUIC packets header | ciphertext | tag.  No call above can express one: its AAD is the packet header, whose length differs
 * from packet to packet; its nonce takes a 62-bit packet number of which only 1 to 4 truncated bytes are on the wire; and those bytes and the low bits of the first byte are
 * masked by header protection, AES-ECB of a 16-byte ciphertext sample under a second key.  aesgcm_keytab_quic_crypt_dev takes the buffer as it is: packet p is bytes
 * [d_pkt_off[p], d_pkt_off[p + 1]) of d_in and of d_out (the same n_pkts + 1 offsets for both; d_in == d_out allowed; any byte alignment), L bytes long: ONE QUIC packet, long
 * or short header, laid out header | payload | tag[16].  Its packet-number field starts at byte d_pn_off[p] (DEVICE memory, n_pkts uint32): the caller parses the unprotected
 * parts of the header (connection-ID lengths, token, Length) to find it.  pn_len = (first byte & 3) + 1, read from the UNPROTECTED first byte; AAD = bytes
 * [0, d_pn_off[p] + pn_len); payload = [d_pn_off[p] + pn_len, L - 16), length 0 is taken.
 * Two slots of the same table per packet.  d_slots[p]: the AEAD -- its key by aesgcm_keytab_set from the `quic key`, its 12-byte IV by aesgcm_keytab_set_tls_iv from the
 * `quic iv` (the same slot state and the same formula as TLS 1.3): nonce = IV XOR (00 00 00 00 | be64(pn)).  d_hp_slots[p]: an ordinary slot set by aesgcm_keytab_set from the
 * `quic hp` key, of which only the round keys are used: mask = AES-ECB of the sample, the 16 bytes at d_pn_off[p] + 4 of the PROTECTED packet (RFC 9001 5.4.2); first byte
 * ^= mask[0] & (first byte & 0x80 ? 0x0f : 0x1f); pn byte i ^= mask[1 + i] for i < pn_len.
 *   ENCRYPT (protect)    d_in holds the unprotected header with the truncated packet number already written by the caller (as a SecY writes its SecTAG), the plaintext, and
 *                        16 bytes of room for the tag.  d_pn[p] (DEVICE memory, n_pkts uint64) is the FULL packet number.  The AEAD runs first, then the mask is taken from
 *                        the fresh ciphertext.  d_pn_out and d_auth are ignored.
 *   DECRYPT (unprotect)  d_in holds the protected packet.  d_pn[p] is the EXPECTED packet number: the largest one received in that packet-number space, plus 1.  The device
 *                        removes header protection, decodes the full number from the truncated one exactly as RFC 9000 Appendix A.3 does (the (1 << 62) guard included),
 *                        writes it to d_pn_out[p] (required; may be d_pn), decrypts, and sets d_auth[p] (required) = 1 iff the tag equals the computed one.  The unmasked
 *                        first byte in d_out shows the caller the Key Phase bit.
 * Out of place every byte of an accepted packet in d_out is defined: the header (encrypt: protected, decrypt: unprotected), the payload, and on decrypt the tag copied.  No
 * byte outside an accepted packet is written.
 * A packet the device cannot take is REFUSED on its own, as a TLS record is: either slot is n_slots or more, unset or cleared; its offsets fall; L > 65535;
 * d_pn_off[p] == 0; d_pn_off[p] + 20 > L (the sample must lie inside the packet, which also guarantees that header and tag fit for every pn_len); on encrypt
 * d_pn[p] >= 2^62.  Nothing of it is written, d_pn_out[p] included; d_pn[p] is not read unless every other test passed; d_auth[p] = 0 on decrypt; and the LOWEST such index
 * goes to aesgcm_keytab_status.  FAIL-CLOSED: aesgcm_wipe_failed_dev(device, n_pkts, d_out, 0, d_pkt_off, d_auth, stream) behind a decrypt.
 * AESGCM_EARG, before the table or a device is touched: t NULL; decrypt not 0 / 1; (n_pkts == 0 is AESGCM_OK;) any of d_slots, d_hp_slots, d_pn, d_pn_off, d_in, d_out,
 * d_pkt_off NULL; decrypt without d_auth or d_pn_out; n_pkts >= 2^31.
 * Two launches per call on `stream`, no scratch memory, capture-safe (CAPTURE, under "key tables" above) and asynchronous: encrypt k_kt_quic (the AEAD; shape and order as aesgcm_keytab_records_crypt_dev) then
 * k_kt_quic_hp (a lane per packet); decrypt the other way round.  Ordering and thread safety as the other key-table calls.
 * OUT OF SCOPE: Retry and Version Negotiation packets; coalesced datagrams (split them: one entry of d_pkt_off per packet); ChaCha20; key derivation (INTEGRATION.md "QUIC
 * packets" says which secret becomes what); choosing the slot from the Key Phase bit (the caller who needs it decrypts out of place and retries the failed packets under the
 * next-phase slot); anti-replay and the expected packet number (not this call's: aesgcm_rxwin_* with AESGCM_RXWIN_EXPECT gives d_pn and takes d_pn_out); routing long packets
 * to the row kernels. */
AESGCM_API int aesgcm_keytab_quic_crypt_dev(aesgcm_keytab *t, int decrypt, size_t n_pkts, const uint32_t *d_slots, const uint32_t *d_hp_slots,
                                 const uint64_t *d_pn, uint64_t *d_pn_out, const uint32_t *d_pn_off,
                                 const void *d_in, const uint64_t *d_pkt_off, void *d_out, int *d_auth, void *stream);

/* ---------------------------------------------------------------- key tables on DTLS RECORDS in wire format: DTLS 1.3 (RFC 9147) and DTLS 1.2 AES-GCM (RFC 6347, RFC 5288)
 * What a WebRTC, VPN or IoT terminator holds is one buffer of DTLS records.  The TLS call cannot express one: a DTLS 1.2 record carries its own epoch and sequence number
 * (its header is 13 bytes, and the AAD takes the number from the wire, not from d_seq), and a DTLS 1.3 record has a header of per-record length whose sequence-number bytes
 * are encrypted -- AES-ECB of a ciphertext sample under a second key, QUIC's structure at other offsets.  aesgcm_keytab_dtls_crypt_dev takes the buffer as it is: record p is
 * bytes [d_rec_off[p], d_rec_off[p + 1]) of d_in and of d_out (the same n_recs + 1 offsets for both; d_in == d_out allowed; any byte alignment), L bytes long, ONE record,
 * under slot d_slots[p].  fmt->version says which record:
 *   AESGCM_DTLS_12  hdr[13] | explicit_nonce[8] | payload | tag[16], hdr = type | version[2] | epoch[2] | sequence number[6] | length[2]  (RFC 6347 4.1, RFC 5288 3).
 *                   Nonce = the slot IV's first four bytes (aesgcm_keytab_set_tls_iv, as TLS 1.2), then the record's bytes [13, 21).  AAD = rec[3..11) (epoch | sequence
 *                   number, FROM THE WIRE) | rec[0..3) | be16(L - 37), 13 bytes; the LENGTH FROM THE OFFSETS -- the header's own two length bytes are not read for it.
 *                   Header and explicit nonce pass through.  ONE launch.  d_sn_slots, d_seq, d_seq_out and d_sn_off are ignored and may be NULL.  Refused beside the
 *                   common refusals: L < 37, L - 13 > 65535.
 *   AESGCM_DTLS_13  unified_hdr | payload | tag[16]  (RFC 9147 4).  The first byte b0 = 0 0 1 C S L E E is never masked.  d_sn_off[p] (DEVICE memory, n_recs uint32) is where
 *                   the sequence-number field starts: 1 + the connection ID's length, which the caller knows and the device does not.  The field is 2 bytes if b0 & 0x08
 *                   (S), else 1; 2 length bytes follow it if b0 & 0x04 (L): hdr = d_sn_off[p] + (S ? 2 : 1) + (L ? 2 : 0).  AAD = rec[0, hdr) with the sequence bytes
 *                   UNPROTECTED.  Payload = [hdr, L - 16), length 0 is taken.  The length field, if present, is not interpreted.  Nonce = the slot's 12-byte IV
 *                   (aesgcm_keytab_set_tls_iv, from the `iv`) XOR (00 00 00 00 | be64(seq)): the TLS 1.3 formula, and seq is the number that the caller passes -- RFC 9147's
 *                   64-bit record sequence number, epoch in the upper 16 bits, is the caller's to form.
 *                   Record-number encryption (RFC 9147 4.2.3): mask = AES-ECB of the 16 bytes rec[hdr, hdr + 16) of the PROTECTED record under the round keys of slot
 *                   d_sn_slots[p], an ordinary slot of the same table set by aesgcm_keytab_set from the `sn` key; sequence byte i ^= mask[i], i < 1 or 2.
 *     ENCRYPT   d_in holds the header with the truncated number already written by the caller, the plaintext, and 16 bytes of room for the tag.  d_seq[p] (DEVICE memory,
 *               n_recs uint64) is the FULL number.  The AEAD launch runs first, then the mask launch on the fresh ciphertext.  d_seq_out and d_auth are ignored.
 *     DECRYPT   d_in holds the protected record.  d_seq[p] is the EXPECTED number.  The mask launch runs first: it unmasks into d_out (out of place it writes the whole
 *               header there) and decodes the full number into d_seq_out[p] (required; may be d_seq).  Then the AEAD launch, which reads the header through d_out and the
 *               number from d_seq_out.
 *     The decode is RFC 9000 Appendix A.3's on 8 or 16 bits: of the numbers whose low bits are the truncated ones, the one closest to the expected number, a tie (exactly
 *     half a window away) going upwards.  No step wraps a 64-bit value: at expected 0 nothing is looked for below zero (an expected 0 and truncated bits t give t), and at
 *     expected 2^64 - 1 nothing above it (the result is the candidate of the last window, (2^64 - 1) with its low bits replaced by the truncated ones).
 *     Refused, by both kernels through the same tests in this order, and reported by the AEAD alone: either slot is n_slots or more, unset or cleared; the offsets fall;
 *     L > 65535; d_sn_off[p] == 0; d_sn_off[p] + 17 > L (only after this test is b0 read); (b0 & 0xE0) != 0x20; hdr + 16 > L (the sample must lie inside the record,
 *     which also guarantees that header and tag fit).
 * Common to both: d_auth[p] (required for decrypt, ignored for encrypt) = 1 iff the record's tag equals the computed one.  Out of place every byte of an accepted record in
 * d_out is defined (the header, the payload, and on decrypt the tag copied).  No byte outside an accepted record is written.  A REFUSED record writes nothing, d_seq_out[p]
 * included; its d_seq[p] is not read; d_auth[p] = 0 on decrypt; and the LOWEST refused index goes to aesgcm_keytab_status.  Common refusals: the slot is n_slots or more,
 * unset or cleared; the offsets fall.  FAIL-CLOSED: aesgcm_wipe_failed_dev(device, n_recs, d_out, 0, d_rec_off, d_auth, stream) behind a decrypt, as for TLS.
 * aesgcm_dtls_fmt_check: AESGCM_EARG for NULL, a version other than AESGCM_DTLS_13 / AESGCM_DTLS_12, reserved != 0.  It touches no device; the crypt call runs it first.
 * Then AESGCM_EARG, before the table or a device is touched, in aesgcm_keytab_quic_crypt_dev's order: t NULL; decrypt not 0 / 1; (n_recs == 0 is AESGCM_OK;) any of d_slots,
 * d_in, d_out, d_rec_off NULL, for 1.3 also d_sn_slots, d_seq, d_sn_off; decrypt without d_auth, for 1.3 also without d_seq_out; n_recs >= 2^31.
 * 1.2: one k_kt_dtls launch; 1.3: two launches on `stream`, k_kt_dtls and k_kt_dtls_sn (a lane per record).  No scratch memory, no host synchronisation, capture-safe (CAPTURE, under "key tables" above) and
 * asynchronous; shape and order as aesgcm_keytab_records_crypt_dev.  Ordering and thread safety as the other key-table calls.
 * OUT OF SCOPE: DTLS 1.2 connection IDs (RFC 9146: another header and another AAD); coalesced datagrams (split them: one entry of d_rec_off per record); choosing the slot
 * from the epoch bits (E E of b0, or a 1.2 header's epoch: the caller maps them to slots); anti-replay (not this call's: aesgcm_rxwin_*, AESGCM_RXWIN_EXPECT for 1.3's d_seq, {WIRE, 5, 6} for 1.2); key derivation (INTEGRATION.md "DTLS records" says which secret
 * becomes what); ChaCha20 and CCM suites; routing long records to the row kernels. */
#define AESGCM_DTLS_13 1u   /* unified_hdr | payload | tag[16]; nonce = slot IV XOR (0^32 | be64(seq)); AAD = the unprotected header; record-number encryption under d_sn_slots[p] */
#define AESGCM_DTLS_12 2u   /* hdr[13] | explicit nonce[8] | payload | tag[16]; nonce = slot IV[0..4) | explicit nonce; AAD = rec[3..11) | rec[0..3) | be16(L - 37) */
typedef struct aesgcm_dtls_fmt {
    uint32_t version;   /* AESGCM_DTLS_13 or AESGCM_DTLS_12 */
    uint32_t reserved;  /* 0                                */
} aesgcm_dtls_fmt;      /* 8 bytes */
AESGCM_API int aesgcm_dtls_fmt_check(const aesgcm_dtls_fmt *fmt);
AESGCM_API int aesgcm_keytab_dtls_crypt_dev(aesgcm_keytab *t, int decrypt, const aesgcm_dtls_fmt *fmt, size_t n_recs, const uint32_t *d_slots, const uint32_t *d_sn_slots,
                                 const uint64_t *d_seq, uint64_t *d_seq_out, const uint32_t *d_sn_off,
                                 const void *d_in, const uint64_t *d_rec_off, void *d_out, int *d_auth, void *stream);

/* ---------------------------------------------------------------- key tables on SRTP AND SRTCP PACKETS in wire format: RFC 7714 AEAD_AES_128_GCM / AEAD_AES_256_GCM
 * A WebRTC terminator uses DTLS for the handshake only: every media byte it moves is SRTP, every control packet SRTCP (RFC 3711).  Under RFC 7714 both are AES-GCM with the
 * nonce and the AAD taken from the packet.  No other call can express them: the RTP header's length is in the packet (CSRC count, X bit, the extension's own length field);
 * the tag is not the packet's last bytes (SRTCP's E-flag / index word and an optional MKI follow it); and SRTCP's AAD is not contiguous (the packet's front plus the word
 * behind the tag).  aesgcm_keytab_srtp_crypt_dev takes the buffer as it is: packet p is bytes [d_pkt_off[p], d_pkt_off[p + 1]) of d_in and of d_out (the same n_pkts + 1
 * offsets for both; d_in == d_out allowed; any byte alignment), L bytes long, ONE packet, under slot d_slots[p].  The slot holds the session key (aesgcm_keytab_set) and the
 * 12-byte session salt (aesgcm_keytab_set_tls_iv: the slot state that TLS, QUIC and DTLS use for their IV).  fmt->mki_len (0 .. 128) bytes of MKI end every packet of the
 * call; they pass through and are not authenticated (RFC 3711 3.1).  fmt->kind says which packet:
 *   AESGCM_SRTP_RTP   rtp_hdr | payload | tag[16] | mki  (RFC 7714 8, 9; RFC 3711 3.1).  hdr = 12 + 4 * (b0 & 15), b0 the first byte; if b0 & 0x10 (the X bit),
 *                     hdr += 4 + 4 * be16(pkt[hdr + 2 .. hdr + 4)), the extension's length taken at the hdr of before.  AAD = pkt[0, hdr).  Payload = [hdr, L - 16 - mki_len),
 *                     length 0 is taken; RTP padding is payload and is not interpreted.  Nonce = salt XOR (00 00 | pkt[8..12) | be32(d_roc[p]) | pkt[2..4)): SSRC, rollover
 *                     counter, sequence number.  d_roc (DEVICE memory, n_pkts numeric uint32) is the rollover counter to use for each packet: a sender passes its own, a
 *                     receiver estimates it from its highest sequence number before the call (RFC 3711 3.3.1), as an XPN receiver does for d_hi.
 *   AESGCM_SRTP_RTCP  rtcp_hdr[8] | payload | tag[16] | W[4] | mki, W = E (1 bit) | index (31 bits), big-endian  (RFC 7714 9.2 - 10; RFC 3711 3.4).  W IS READ FROM THE WIRE
 *                     in both directions: the sender writes W and the headers before the call, as a SecY writes its SecTAG.  Nonce = salt XOR (00 00 | pkt[4..8) | 00 00 |
 *                     be32(W & 0x7FFFFFFF)).  E = 1: AAD = pkt[0, 8) | W, 12 bytes; payload = [8, L - 20 - mki_len).  E = 0: nothing is encrypted; AAD = pkt[0, L - 20 -
 *                     mki_len) | W, and every byte passes through.  E is per packet: one call mixes both.  d_roc is ignored and may be NULL.
 * d_auth[p] (required for decrypt, ignored for encrypt) = 1 iff the packet's tag equals the computed one.  Out of place every byte of an accepted packet in d_out is defined:
 * what is not ciphertext or plaintext is copied -- the header, W, the MKI, and on decrypt the tag's bytes as they came.  No byte outside an accepted packet is written.
 * A REFUSED packet is left untouched; d_auth[p] = 0 on decrypt; the LOWEST refused index goes to aesgcm_keytab_status; the rest of the call runs.  Its bytes and its d_roc[p]
 * are not read past the test that refuses it.  The tests, in this order: the slot is n_slots or more, unset or cleared; the offsets fall; L > 65535; L < 12 + 16 + mki_len
 * (RTP) or L < 8 + 20 + mki_len (RTCP); only now is b0 read: (b0 & 0xC0) != 0x80; RTP: hdr + 16 + mki_len > L behind the CSRC term; with X: hdr + 4 + 16 + mki_len > L,
 * tested before the extension's length is read; with X: hdr + 16 + mki_len > L behind the extension.
 * FAIL-CLOSED: aesgcm_wipe_failed_dev(device, n_pkts, d_out, 0, d_pkt_off, d_auth, stream) behind a decrypt, as for TLS.
 * aesgcm_srtp_fmt_check: AESGCM_EARG for NULL, a kind other than AESGCM_SRTP_RTP / AESGCM_SRTP_RTCP, mki_len > 128.  It touches no device; the crypt call runs it first.
 * Then AESGCM_EARG, before the table or a device is touched, in aesgcm_keytab_dtls_crypt_dev's order: t NULL; decrypt not 0 / 1; (n_pkts == 0 is AESGCM_OK;) any of d_slots,
 * d_in, d_pkt_off, d_out NULL; RTP without d_roc; decrypt without d_auth; n_pkts >= 2^31.
 * ONE k_kt_srtp launch: no scratch memory, no host synchronisation, capture-safe (CAPTURE, under "key tables" above) and asynchronous; shape, order and planning as aesgcm_keytab_dtls_crypt_dev's DTLS 1.2
 * mode.  Ordering and thread safety as the other key-table calls.
 * OUT OF SCOPE: ROC estimation and replay windows (not this call's: aesgcm_rxwin_recover_dev with AESGCM_RXWIN_SRTP writes d_roc, aesgcm_rxwin_commit_dev keeps the window); the DTLS-SRTP exporter (not this call's: aesgcm_prf12_export_srtp_dev under "TLS 1.2 PRF" below fills the master table on the device; without it the master key and salt are the caller's: INTEGRATION.md "SRTP and SRTCP packets" says which secret
 * becomes what -- the session key derivation from them, RFC 3711 4.3, is aesgcm_srtp_kdf_* under "SRTP KEY DERIVATION" below); the AES-CM / HMAC-SHA1 transforms; double encryption (RFC 8723); RFC 6904 header-extension encryption; MKI lookup (the caller maps an MKI to a slot, and one
 * call has one mki_len); splitting reduced-size or multiplexed datagrams (one entry of d_pkt_off per packet; a compound RTCP packet is ONE packet). */
#define AESGCM_SRTP_RTP  1u
#define AESGCM_SRTP_RTCP 2u
typedef struct aesgcm_srtp_fmt {
    uint32_t kind;      /* AESGCM_SRTP_RTP or AESGCM_SRTP_RTCP */
    uint32_t mki_len;   /* 0 .. 128: bytes of MKI that end the packet, passed through, not authenticated */
} aesgcm_srtp_fmt;      /* 8 bytes */
AESGCM_API int aesgcm_srtp_fmt_check(const aesgcm_srtp_fmt *fmt);
AESGCM_API int aesgcm_keytab_srtp_crypt_dev(aesgcm_keytab *t, int decrypt, const aesgcm_srtp_fmt *fmt, size_t n_pkts,
                                 const uint32_t *d_slots, const uint32_t *d_roc,
                                 const void *d_in, const uint64_t *d_pkt_off, void *d_out, int *d_auth, void *stream);

/* ---------------------------------------------------------------- key tables on SSH BINARY PACKETS in wire format: RFC 5647 AEAD_AES_128_GCM / AEAD_AES_256_GCM
 * An SSH bastion, an SFTP front end or a Git host holds thousands of connections, each with its own key, and one buffer of short packets.  Under
 * aes128-gcm@openssh.com / aes256-gcm@openssh.com (OpenSSH PROTOCOL 1.6) and RFC 5647's AEAD_AES_128_GCM / AEAD_AES_256_GCM (7.2, 7.3) a packet is
 *   packet_length[4] | body[B] | tag[16]        B = L - 20
 * packet_length in the clear, the AAD's four bytes; body = padding_length, payload and padding, not interpreted; B a whole number of cipher blocks and at least one.
 * No other call can express it: no nonce byte is on the wire, and the nonce is not an XOR.  aesgcm_keytab_ssh_crypt_dev takes the buffer as it is: packet p is bytes
 * [d_pkt_off[p], d_pkt_off[p + 1]) of d_in and of d_out (the same n_pkts + 1 offsets for both; d_in == d_out allowed; any byte alignment), L bytes long, under slot
 * d_slots[p].  The slot holds the direction's encryption key (aesgcm_keytab_set) and its 12-byte initial IV (aesgcm_keytab_set_tls_iv: the slot state that TLS, QUIC,
 * DTLS and SRTP use): fixed[4] | invocation_counter[8] (RFC 5647 7.1).
 *   NONCE = fixed[4] | be64((be64(invocation_counter) + d_seq[p]) mod 2^64)
 * d_seq[p] (DEVICE memory, n_pkts numeric 64-bit values, as TLS 1.3's) is the number of packets sent under this key before this one.  It is ADDED, with its carries
 * through all 64 bits of the counter; the carry never runs into the fixed field.  (SSH's 32-bit implicit sequence number is not used by AES-GCM and is not this value:
 * d_seq restarts at 0 with every key.)
 * Encrypt writes the body and the tag; THE CALLER WROTE packet_length, as it writes a TLS header.  Decrypt writes the body and d_auth[p] = 1 iff the packet's tag equals
 * the computed one (d_auth is required for decrypt and ignored for encrypt).  Out of place every byte of an accepted packet in d_out is defined: the length field is
 * copied, and on decrypt the tag.  No byte outside an accepted packet is written.
 * A packet is REFUSED on its own.  The tests, in this order: the slot is n_slots or more; the offsets fall; L >= 2^28; L < 36 (the body is at least one cipher block, RFC
 * 5647 7.2); B % 16 != 0; the slot is unset or cleared; be32(packet_length) != B -- ONLY HERE IS THE FIELD READ, in both directions.  Nothing of a refused packet is read
 * past the test that refuses it, nothing of it is written, d_seq[p] is not read, d_auth[p] = 0 on decrypt, and the LOWEST such index goes to aesgcm_keytab_status.
 * FAIL-CLOSED: aesgcm_wipe_failed_dev(device, n_pkts, d_out, 0, d_pkt_off, d_auth, stream) behind a decrypt, as for TLS.
 * AESGCM_EARG for d_seq == NULL, before the call looks at the table; then, in aesgcm_keytab_records_crypt_dev's order: t NULL; decrypt not 0 / 1; (n_pkts == 0 is
 * AESGCM_OK;) any of d_slots, d_in, d_pkt_off, d_out NULL; decrypt without d_auth; n_pkts >= 2^31.
 * ONE k_kt_ssh launch: no scratch memory, no host synchronisation, capture-safe (CAPTURE, under "key tables" above) and asynchronous; shape, order and planning as
 * aesgcm_keytab_records_crypt_dev.  Ordering and thread safety as the other key-table calls.
 * OUT OF SCOPE: chacha20-poly1305@openssh.com; encrypt-then-MAC, CBC and CTR suites; SSH's 32-bit implicit sequence number; finding the packets' boundaries in a TCP
 * stream (the clear length fields are the caller's to walk: one entry of d_pkt_off per packet); compression; the key exchange and the computation of H (the keys from
 * K and H: aesgcm_sshkdf_* under "SSH KEY DERIVATION" below); counting packets (the send counters' business: aesgcm_txnum_assign_dev under "SEND COUNTERS" below gives d_seq --
 * INTEGRATION.md "SSH packets"); routing long packets to the row kernels. */
AESGCM_API int aesgcm_keytab_ssh_crypt_dev(aesgcm_keytab *t, int decrypt, size_t n_pkts, const uint32_t *d_slots, const uint64_t *d_seq,
                                const void *d_in, const uint64_t *d_pkt_off, void *d_out, int *d_auth, void *stream);

/* ---------------------------------------------------------------- RECEIVE WINDOWS: anti-replay and number recovery on the device, for every wire format above
 * A receiver needs, BEFORE a decrypt call, a per-packet value that depends on per-association state -- ESN's seq-hi, XPN's upper PN half, SRTP's rollover counter, the
 * expected number of QUIC and DTLS 1.3 -- and AFTER it must drop replays and advance that state.  aesgcm_rxwin is that state on the device: n_wins independent windows
 * of `window` bits each (a power of two, 64 .. 4096).  A window belongs to whatever the protocol numbers: a MACsec SA, an ESP SA, a DTLS epoch, a QUIC packet-number
 * space, an SRTP SSRC.  It is NOT tied to a key slot (SRTP shares a key across SSRCs, QUIC keeps its number space across key updates): calls name a window per packet
 * with d_win[p] (DEVICE memory, uint32), which is often the same array as d_slots.
 * A window's state: `next`, a uint64 = the highest accepted number + 1, or 0 if nothing was accepted yet; and the set of SEEN numbers in [next - window, next), clamped
 * at 0.  Numbers are 0 .. 2^64 - 2; 2^64 - 1 is AESGCM_RXWIN_NONE, "no number".
 *   aesgcm_rxwin_create   all windows empty.  AESGCM_EARG for a window that is no power of two in 64 .. 4096, n_wins == 0 or n_wins >= 2^31.
 *   aesgcm_rxwin_set      HOST arrays into windows first .. first + n - 1: next[n], and seen[n][window / 64] or NULL for "nothing seen".  The form is NORMALISED and says
 *                         nothing about how the device stores it: bit i of a window's little-endian bit string (bit i & 63 of word i / 64) says "number next - 1 - i was
 *                         seen".  Bits for numbers below 0 must be 0 (AESGCM_EARG).  Stream-ordered through a staging buffer, like aesgcm_keytab_set.
 *   aesgcm_rxwin_get      the same form back (seen may be NULL).  It WAITS on `stream`.  For tests and checkpoints.
 *   aesgcm_rxwin_status   as aesgcm_keytab_status: the LOWEST packet index a recover or commit call refused since the last read, which clears it.
 *   aesgcm_rxwin_destroy  waits for the device, frees.
 * RECOVER, before the decrypt: aesgcm_rxwin_recover_dev writes d_num_out[p] (required, uint64: the packet's full number) and d_hi_out[p] (optional, uint32).  *fmt says
 * where the truncated number lies in packet p = bytes [d_pkt_off[p], d_pkt_off[p + 1]) of d_in and how the full one is formed; T = the window's next, W = window, t = the
 * big-endian field of num_len bytes at byte num_off:
 *   AESGCM_RXWIN_WIRE     num_len 2, 4, 6 or 8.  full = t.  AESGCM_RXWIN_FROM_END: the field starts num_off bytes before the packet's END.  AESGCM_RXWIN_CLEAR_TOP: the
 *                         field's top bit is cleared.  d_hi_out[p] = full >> 32.  MACsec {WIRE, 16, 4}; ESP {WIRE, 4, 4}; DTLS 1.2 {WIRE, 5, 6} (a window is an epoch);
 *                         SRTCP {WIRE, 4 + mki_len, 4, FROM_END | CLEAR_TOP} (the index without its E bit).
 *   AESGCM_RXWIN_LOWEST   num_len 2 or 4.  full = the smallest n >= B with n = t (mod 2^(8 num_len)), B = T >= W ? T - W : 0: the number is taken to lie at or above the
 *                         lowest acceptable one (RFC 4303 Appendix A2.1, 802.1AEbw 10.6.2).  d_hi_out[p] = full >> (8 num_len) (its low 32 bits), which is exactly the
 *                         d_hi of aesgcm_keytab_frames_crypt_x_dev.  ESN {LOWEST, 4, 4}; XPN {LOWEST, 16, 4}.
 *   AESGCM_RXWIN_SRTP     num_len 2 (RTP: num_off 2).  RFC 3711 3.3.1 and Appendix A on s_l = (T - 1) & 0xFFFF, ROC = (T - 1) >> 16: if s_l < 32768, v = ROC - 1 when
 *                         SEQ - s_l > 32768, else ROC; otherwise v = ROC + 1 when s_l - 32768 > SEQ, else ROC.  Nothing goes below ROC 0: then v stays 0.  T == 0 gives
 *                         v = 0 (a receiver that joins mid-stream uses aesgcm_rxwin_set first).  full = v << 16 | SEQ; d_hi_out[p] = v is aesgcm_keytab_srtp_crypt_dev's d_roc.
 *   AESGCM_RXWIN_EXPECT   num_len 0.  No packet byte is read; d_in and d_pkt_off may be NULL.  d_num_out[p] = T: the d_pn / d_seq that the QUIC and DTLS 1.3 decrypt calls
 *                         take as the EXPECTED number (d_hi_out[p] = T >> 32).  Their d_pn_out / d_seq_out then go to the commit as d_num.
 * A packet is REFUSED on its own when its window is n_wins or more; (EXPECT: T is 2^64 - 1;) its offsets fall; its number field is not inside the packet; the result would
 * be 2^64 - 1 or more; the rollover counter would pass 2^32 - 1.  The tests run in this order and nothing of the packet is read past the one that refuses it.  Then
 * d_num_out[p] = AESGCM_RXWIN_NONE, d_hi_out[p] = 0xFFFFFFFF, and the lowest such index goes to aesgcm_rxwin_status.  Recover changes no window.
 * aesgcm_rxwin_fmt_check: AESGCM_EARG for NULL, an unknown rule or flag, a num_len the rule does not take, flags on a rule other than WIRE, num_off >= 2^16.  It touches no
 * device; the recover call runs it first, then AESGCM_EARG for w NULL, (n_pkts == 0 is AESGCM_OK,) d_win or d_num_out NULL, d_in or d_pkt_off NULL unless EXPECT,
 * n_pkts >= 2^31 -- all before any device is touched.
 * COMMIT, behind the decrypt: aesgcm_rxwin_commit_dev(w, n_pkts, d_win, d_num, d_auth, d_accept, d_why).  S = the call's packets with d_auth[p] != 0, d_win[p] < n_wins and
 * d_num[p] != AESGCM_RXWIN_NONE.  Per window M = max(next, 1 + the largest d_num in S).  A packet of S is
 *   OLD      if num + W < M;
 *   REPLAY   if it is not old and its number was seen before the call, or another packet of S with the same window and number is accepted;
 *   ACCEPT   otherwise: of the non-old packets of one (window, number) not seen before, EXACTLY ONE is accepted -- which one is unspecified (they authenticated under
 *            one key and nonce).
 * Afterwards next = M and seen = (seen before, and the accepted) within [M - W, M).  This is RFC 4303 A2's sequential check-and-update applied to the call's
 * authenticated packets in DESCENDING number order: the window advances first.  No number is ever accepted twice, across any sequence of calls.  A packet with
 * d_auth[p] == 0 changes nothing, whatever its number: a forgery cannot move a window.  A call that spans more than W numbers loses its oldest: SIZE `window` FOR THE
 * REORDERING YOU TOLERATE PLUS THE SPAN OF ONE CALL.
 * d_accept[p] (required) = 1 or 0; it MAY BE d_auth, and aesgcm_wipe_failed_dev on it then wipes replays as it wipes forgeries.  d_why[p] (optional, int) = 0 not
 * authenticated, 1 accepted, 2 old, 3 replay, 4 refused: authenticated, but its window is out of range or its number is NONE; the lowest such index goes to
 * aesgcm_rxwin_status.  AESGCM_EARG, before any device is touched: w NULL; (n_pkts == 0 is AESGCM_OK;) d_win, d_num, d_auth or d_accept NULL; n_pkts >= 2^31.
 * One launch per recover, three per commit (the per-window maximum; clearing what the window moves over; marking), a lane per packet, atomics on the window's own words: no
 * scratch memory, no host synchronisation, capture-safe (CAPTURE, under "key tables" above: the precondition, what a graph holds) and asynchronous on `stream`.  Every call but aesgcm_rxwin_get is stream-ordered; two calls that name the same
 * window on different streams are the caller's to order; the calls of one table are thread-safe; a table belongs to the device it was created on.
 * OUT OF SCOPE: skipping the decryption of packets a pre-check could already reject; per-window counters; MACsec's replayProtect = false mode; choosing a window from a
 * wire field (SCI, SPI, SSRC lookup); TLS, which has no replay window. */
#define AESGCM_RXWIN_NONE 0xFFFFFFFFFFFFFFFFull   /* "no number" */
#define AESGCM_RXWIN_WIRE   1u   /* full = the wire field */
#define AESGCM_RXWIN_LOWEST 2u   /* full = the smallest number at or above next - window with the wire field's low bits */
#define AESGCM_RXWIN_SRTP   3u   /* full = ROC estimate << 16 | SEQ (RFC 3711 Appendix A) */
#define AESGCM_RXWIN_EXPECT 4u   /* d_num_out = next; no packet byte is read */
#define AESGCM_RXWIN_FROM_END  1u   /* WIRE: the field starts num_off bytes before the packet's end */
#define AESGCM_RXWIN_CLEAR_TOP 2u   /* WIRE: the field's top bit is cleared */
typedef struct aesgcm_rxwin aesgcm_rxwin;
typedef struct aesgcm_rxwin_fmt {
    uint32_t rule;      /* AESGCM_RXWIN_WIRE, _LOWEST, _SRTP or _EXPECT                      */
    uint32_t num_off;   /* where the truncated number starts (FROM_END: before the end), < 2^16 */
    uint32_t num_len;   /* its bytes: WIRE 2 / 4 / 6 / 8, LOWEST 2 / 4, SRTP 2, EXPECT 0        */
    uint32_t flags;     /* WIRE: 0 or AESGCM_RXWIN_FROM_END | AESGCM_RXWIN_CLEAR_TOP; else 0    */
} aesgcm_rxwin_fmt;     /* 16 bytes */
AESGCM_API int aesgcm_rxwin_create(aesgcm_rxwin **out, int device, size_t n_wins, size_t window);
AESGCM_API int aesgcm_rxwin_set(aesgcm_rxwin *w, size_t first, size_t n, const uint64_t *next, const uint64_t *seen, void *stream);
AESGCM_API int aesgcm_rxwin_get(aesgcm_rxwin *w, size_t first, size_t n, uint64_t *next, uint64_t *seen, void *stream);
AESGCM_API int aesgcm_rxwin_fmt_check(const aesgcm_rxwin_fmt *fmt);
AESGCM_API int aesgcm_rxwin_recover_dev(aesgcm_rxwin *w, const aesgcm_rxwin_fmt *fmt, size_t n_pkts, const uint32_t *d_win, const void *d_in, const uint64_t *d_pkt_off,
                             uint64_t *d_num_out, uint32_t *d_hi_out, void *stream);
AESGCM_API int aesgcm_rxwin_commit_dev(aesgcm_rxwin *w, size_t n_pkts, const uint32_t *d_win, const uint64_t *d_num, const int *d_auth, int *d_accept, int *d_why,
                            void *stream);
AESGCM_API int aesgcm_rxwin_status(aesgcm_rxwin *w, int *code, uint64_t *detail);
AESGCM_API int aesgcm_rxwin_destroy(aesgcm_rxwin *w);

/* ---------------------------------------------------------------- SEND COUNTERS: packet numbers handed out on the device, in packet order, for every wire format above
 * A sender needs, BEFORE an encrypt call, a fresh number per packet from per-association state -- and that state must never go wrong: a number used twice under one key
 * gives away the authentication key.  aesgcm_txnum is that state on the device: n_ctrs independent counters.  A counter is `next` (uint64: the number the next packet
 * gets) and `limit` (uint64, EXCLUSIVE: only numbers below limit are ever handed out; limit is at most 2^64 - 1, so AESGCM_RXWIN_NONE is never a number).  Like a
 * receive window a counter belongs to whatever the protocol numbers and is NOT tied to a key slot: calls name a counter per packet with d_ctr[p] (DEVICE memory,
 * uint32), which often holds the same numbers as d_slots (in an array of its own: see d_slots below).
 *   aesgcm_txnum_create   every counter next = 0, limit = 0: an unset counter refuses everything.  All scratch memory an assign call needs is allocated HERE, sized by
 *                         max_pkts: a call allocates nothing.  AESGCM_EARG for n_ctrs == 0, n_ctrs >= 2^31, max_pkts == 0, max_pkts >= 2^31.
 *   aesgcm_txnum_set      HOST arrays next[n], limit[n] into counters first .. first + n - 1.  AESGCM_EARG for next[k] > limit[k].  Stream-ordered through a staging
 *                         buffer, like aesgcm_rxwin_set.
 *   aesgcm_txnum_get      the same arrays back (limit may be NULL).  It WAITS on `stream`.  For tests, checkpoints and rekey polling (rekey when limit - next runs low).
 *   aesgcm_txnum_status   as aesgcm_rxwin_status: the LOWEST packet index an assign call refused since the last read, which clears it.
 *   aesgcm_txnum_destroy  waits for the device, frees.
 * ASSIGN, before the encrypt: aesgcm_txnum_assign_dev(t, fmt, n_pkts, d_ctr, d_pkts, d_pkt_off, d_num_out, d_hi_out, d_slots, stream).
 * ORDER: the packets of one call that name counter c, taken in ASCENDING ARRAY INDEX, get next_c, next_c + 1, ...; afterwards next_c has grown by their count, capped at
 * limit_c.  The result is deterministic, and no number is handed out twice, across any sequence of calls on one stream.  (Receivers' windows are sized for the
 * network's reordering, not for a shuffled call.)
 * d_num_out[p] (required, uint64) is the full number: the d_seq / d_pn of the TLS 1.3, QUIC and DTLS 1.3 calls.  d_hi_out[p] (optional, uint32) = num >> 32: the d_hi of
 * aesgcm_keytab_frames_crypt_x_dev.  *fmt says what is written into packet p = bytes [d_pkt_off[p], d_pkt_off[p + 1]) of d_pkts, IN PLACE, before the encrypt: the low
 * num_len bytes of the number, big-endian, at byte num_off.  num_len is 0, 2, 4, 6 or 8; with 0 no packet byte is written and d_pkts / d_pkt_off may be NULL (TLS 1.3,
 * QUIC, DTLS 1.3: their calls place their own bytes).  dup_off != 0 writes the same bytes a second time at dup_off.
 *   AESGCM_TXNUM_FROM_END  num_off and dup_off count back from the packet's END, as AESGCM_RXWIN_FROM_END does.
 *   AESGCM_TXNUM_KEEP_TOP  the field's top bit is left as it is and the number takes 8 num_len - 1 bits (SRTCP's E bit).
 *   AESGCM_TXNUM_WHOLE     the field is the WHOLE number: a number that does not fit the field's bits refuses the packet.  The fail-closed stop of classic MACsec and
 *                          ESP at 2^32, whatever `limit` says.
 *   MACsec {16, 4, 0, WHOLE}; MACsec XPN {16, 4, 0, 0}; ESP {4, 4, 0, WHOLE}; ESP ESN {4, 4, 0, 0}; TLS 1.2 {5, 8, 0, WHOLE} (the explicit nonce); DTLS 1.2
 *   {5, 6, 15, WHOLE} (the record's sequence number, and again as the sequence half of the explicit nonce; the epoch bytes of both are the caller's); SRTCP
 *   {4 + mki_len, 4, 0, FROM_END | KEEP_TOP | WHOLE}; number only {0, 0, 0, 0}.
 * A packet is REFUSED on its own, by these tests in this order, and no packet byte is touched past the one that refuses: (1) d_ctr[p] >= n_ctrs; (2) its number would be
 * at or above limit; (3) WHOLE and the number does not fit; (4) falling offsets; (5) the field or its duplicate not inside the packet.  Then d_num_out[p] =
 * AESGCM_RXWIN_NONE, d_hi_out[p] = 0xFFFFFFFF, none of its bytes is written, and, if d_slots (optional, uint32, in/out) is given, d_slots[p] = 0xFFFFFFFF: the encrypt
 * call behind refuses exactly these packets and never encrypts under a number that was not granted.  d_slots MUST NOT BE d_ctr, however equal their contents: the
 * entry of a refused packet is overwritten while other lanes still read the counter numbers.  The lowest such index goes to aesgcm_txnum_status.  A packet
 * refused by tests 3 to 5 HAS BEEN COUNTED: its number is BURNT, not reused.
 * aesgcm_txnum_fmt_check: AESGCM_EARG for NULL, an unknown flag, a num_len other than 0 / 2 / 4 / 6 / 8, num_off or dup_off >= 2^16, a duplicate that overlaps the
 * field, KEEP_TOP, WHOLE or dup_off with num_len == 0.  It touches no device; the assign call runs it first, then AESGCM_EARG for t NULL, (n_pkts == 0 is AESGCM_OK,)
 * d_ctr or d_num_out NULL, d_pkts or d_pkt_off NULL with num_len != 0, n_pkts > max_pkts -- all before any device is touched.
 * The call is a stable radix sort of the packet indices by counter (three launches per 8 bits of n_ctrs: one pass up to 255 counters, two up to 65 535) and two
 * launches a lane per packet; no workgroup waits for another, and no atomic but the status word's: the cost does not depend on how many packets share a counter.  Its
 * launch sequence is fixed for given n_pkts and table; no allocation, no host synchronisation, nothing read back: capture-safe (CAPTURE, under "key tables" above) and
 * asynchronous on `stream`.  Every call but aesgcm_txnum_get is stream-ordered.  TWO ASSIGN CALLS OF ONE TABLE MUST NOT RUN CONCURRENTLY on different streams -- they
 * share the table's scratch, whichever counters they name: the caller orders them.  The host calls of one table are thread-safe; a table belongs to its device.
 * OUT OF SCOPE: SRTP's sequence number (the application's) and its rollover counter (the caller's); DTLS epochs and the epoch bytes; choosing a counter from a wire
 * field; a single-launch path for small calls. */
#define AESGCM_TXNUM_FROM_END 1u   /* num_off / dup_off count back from the packet's end */
#define AESGCM_TXNUM_KEEP_TOP 2u   /* the field's top bit is left as it is; the number takes 8 num_len - 1 bits */
#define AESGCM_TXNUM_WHOLE    4u   /* the field is the whole number: one that does not fit refuses the packet */
typedef struct aesgcm_txnum aesgcm_txnum;
typedef struct aesgcm_txnum_fmt {
    uint32_t num_off;   /* where the number's field starts (FROM_END: before the end), < 2^16 */
    uint32_t num_len;   /* its bytes: 0 (nothing is written), 2, 4, 6 or 8                     */
    uint32_t dup_off;   /* 0, or where the same bytes are written a second time, < 2^16       */
    uint32_t flags;     /* AESGCM_TXNUM_FROM_END | AESGCM_TXNUM_KEEP_TOP | AESGCM_TXNUM_WHOLE  */
} aesgcm_txnum_fmt;     /* 16 bytes */
AESGCM_API int aesgcm_txnum_create(aesgcm_txnum **out, int device, size_t n_ctrs, size_t max_pkts);
AESGCM_API int aesgcm_txnum_set(aesgcm_txnum *t, size_t first, size_t n, const uint64_t *next, const uint64_t *limit, void *stream);
AESGCM_API int aesgcm_txnum_get(aesgcm_txnum *t, size_t first, size_t n, uint64_t *next, uint64_t *limit, void *stream);
AESGCM_API int aesgcm_txnum_fmt_check(const aesgcm_txnum_fmt *fmt);
AESGCM_API int aesgcm_txnum_assign_dev(aesgcm_txnum *t, const aesgcm_txnum_fmt *fmt, size_t n_pkts, const uint32_t *d_ctr, void *d_pkts, const uint64_t *d_pkt_off,
                            uint64_t *d_num_out, uint32_t *d_hi_out, uint32_t *d_slots, void *stream);
AESGCM_API int aesgcm_txnum_status(aesgcm_txnum *t, int *code, uint64_t *detail);
AESGCM_API int aesgcm_txnum_destroy(aesgcm_txnum *t);

/* ---------------------------------------------------------------- ON-DEVICE KEY DERIVATION: TLS 1.3, QUIC and DTLS 1.3 keys from traffic secrets that never leave the device
 * In TLS 1.3 (RFC 8446 7.3), QUIC (RFC 9001 5.1, RFC 9369 3.3.2) and DTLS 1.3 (RFC 9147 5.9) a direction's AEAD key, its IV and its header-protection / record-number
 * key all come from ONE traffic secret by HKDF-Expand-Label, and the next generation's secret comes from this one the same way (RFC 8446 7.2, RFC 9001 6).
 * aesgcm_kdf is a table of n_secrets such secrets on the device, of one hash: hash_len 32 = SHA-256, 48 = SHA-384.  No call reads a secret back.  THE TABLE HOLDS
 * TRAFFIC SECRETS: PROTECT IT LIKE KEYS -- whoever holds a secret holds every key of its generation and of all later ones.
 *   aesgcm_kdf_create     every record unset.  AESGCM_EARG for a hash_len other than 32 / 48, n_secrets == 0 or >= 2^31.
 *   aesgcm_kdf_set        HOST secrets (n * hash_len bytes) into records first .. first + n - 1, through the table's staging buffer on `stream`, which is zeroed
 *                         behind the copy as aesgcm_keytab_set zeroes its keys; the library's host copy is wiped before the call returns.
 *   aesgcm_kdf_set_dev    n secrets from DEVICE memory (n * hash_len bytes, no alignment asked) into the records d_idx[i]; an index out of range is refused.
 *   aesgcm_kdf_clear      records first .. first + n - 1 zeroed and unset.
 *   aesgcm_kdf_status     as aesgcm_keytab_status: the LOWEST entry index an install, update or set_dev call refused since the last read, which clears it.
 *   aesgcm_kdf_destroy    waits for the device, zeroes the records and the staging buffer, frees.
 * A FORMAT names the four labels in full, prefix included ("tls13 key", "tls13 quic hp", "dtls13sn"): 0 the key, 1 the IV, 2 the auxiliary key (QUIC's hp, DTLS 1.3's
 * sn), 3 the update; len 0 = the protocol has none.  aesgcm_kdf_fmt_check: AESGCM_EARG for NULL, a label longer than 20 bytes, no label 0.  It touches no device.
 * THE BOUND: only HKDF-Expand-Label(secret, label, "", L) with L <= hash_len is computed.  With a label of at most 20 bytes the HMAC's message is at most 25 bytes and
 * every HMAC is exactly four compressions (csrc/aesgcm_kdf.h); the kernels rely on the check and do not repeat it.
 * INSTALL: aesgcm_kdf_install_dev(k, fmt, keytab, n, d_idx, d_slots, d_aux_slots, stream).  For entry i with the secret s of record d_idx[i]:
 *   slot d_slots[i] of `keytab` becomes exactly what aesgcm_keytab_set_dev makes of Expand-Label(s, label 0, key_len) -- round keys, H, its powers, the set marker --
 *   and its TLS-IV field what aesgcm_keytab_set_tls_iv makes of Expand-Label(s, label 1, 12);
 *   with d_aux_slots != NULL and d_aux_slots[i] != 0xFFFFFFFF, slot d_aux_slots[i] is set from Expand-Label(s, label 2, key_len).
 * The table's key size may be 16, 24 or 32 with either hash.  AESGCM_EARG for a format without label 1, for d_aux_slots with a format that has no label 2, and for a key
 * table of another device.  A key update passes d_aux_slots = NULL: QUIC's hp key and DTLS 1.3's sn key do not change with the generation.
 * UPDATE: aesgcm_kdf_update_dev(k, fmt, n, d_from, d_to, stream): rec[d_to[i]] = Expand-Label(rec[d_from[i]], label 3, hash_len), marked set.  d_to[i] == d_from[i] is the
 * update in place (the lane holds the whole secret before it writes).  Two entries of one call that name the same d_to, or an entry whose d_from is another entry's d_to,
 * are the caller's error: that record is unspecified.  An endpoint that keeps the current and the next generation uses two records.
 * REFUSED ENTRIES are skipped whole -- NOTHING an entry names is written -- when d_idx[i], d_from[i] or d_to[i] is out of range, the source record is unset or
 * cleared, d_slots[i] is out of range, or an aux slot other than 0xFFFFFFFF is out of range.  The lowest such index goes to the SECRET table's status word; the key
 * table's status is not touched.
 * NO DERIVED KEY IN MEMORY: a derived key or IV is stored nowhere but in the slot's fields (a new secret: in its record).  The lane that expands a key runs the key
 * schedule itself, from its registers.
 * One launch per call, a lane per derived value (k_kdf_install: entries x {key, iv, aux}, k_kdf_update); no allocation, no event, no host synchronisation, nothing
 * read back: install and update are capture-safe (CAPTURE, under "key tables" above) and asynchronous on `stream`.  Every call is stream-ordered on `stream`; an
 * install on one stream and a crypt call on another that names the slot are the caller's to order, as with aesgcm_keytab_set.  So the key-update loop runs as launches
 * on one stream: aesgcm_txnum_assign_dev refuses at the limit, update, install into a fresh slot, reset the counter, encrypt (INTEGRATION.md "Key derivation").
 * The host calls of one table are thread-safe; a table belongs to its device.
 * OUT OF SCOPE: HKDF-Extract and the handshake key schedule (the traffic secrets are the caller's); the TLS 1.2 PRF (not this table's: aesgcm_prf12_* under "TLS 1.2 PRF" below); IKEv2's prf+ (not this table's: aesgcm_prfplus_* under "IKEv2 PRF+" below); ChaCha20 and CCM suites; the QUIC Initial salt step (RFC 9001 5.2); labels with a context; outputs longer than the hash.  (SRTP's AES-CM key
 * derivation, RFC 3711 4.3, is no HKDF and has a table of its own: aesgcm_srtp_kdf_*, "SRTP KEY DERIVATION" below.) */
typedef struct aesgcm_kdf aesgcm_kdf;
typedef struct aesgcm_kdf_fmt {
    uint8_t len[4];         /* bytes of each label, 0 = absent, at most 20                                  */
    uint8_t label[4][20];   /* full labels, prefix included: 0 key, 1 iv, 2 aux (hp / sn), 3 update        */
} aesgcm_kdf_fmt;           /* 84 bytes */
AESGCM_API int aesgcm_kdf_create(aesgcm_kdf **out, int device, size_t hash_len, size_t n_secrets);
AESGCM_API int aesgcm_kdf_set(aesgcm_kdf *k, size_t first, size_t n, const uint8_t *secrets, void *stream);
AESGCM_API int aesgcm_kdf_set_dev(aesgcm_kdf *k, size_t n, const uint32_t *d_idx, const void *d_secrets, void *stream);
AESGCM_API int aesgcm_kdf_clear(aesgcm_kdf *k, size_t first, size_t n, void *stream);
AESGCM_API int aesgcm_kdf_fmt_check(const aesgcm_kdf_fmt *fmt);
AESGCM_API int aesgcm_kdf_install_dev(aesgcm_kdf *k, const aesgcm_kdf_fmt *fmt, aesgcm_keytab *keytab, size_t n, const uint32_t *d_idx, const uint32_t *d_slots,
                           const uint32_t *d_aux_slots, void *stream);
AESGCM_API int aesgcm_kdf_update_dev(aesgcm_kdf *k, const aesgcm_kdf_fmt *fmt, size_t n, const uint32_t *d_from, const uint32_t *d_to, void *stream);
AESGCM_API int aesgcm_kdf_status(aesgcm_kdf *k, int *code, uint64_t *detail);
AESGCM_API int aesgcm_kdf_destroy(aesgcm_kdf *k);

/* ---------------------------------------------------------------- SRTP KEY DERIVATION: SRTP and SRTCP session keys from master keys that never leave the device
 * An SRTP stream has ONE master key and master salt (from the DTLS-SRTP exporter or SDES: the caller's) and two derived sets of session keys, one for SRTP and one for
 * SRTCP, which a non-zero key_derivation_rate derives anew periodically (RFC 3711 4.3).  aesgcm_srtp_kdf is a table of n_masters such master keys and salts on the
 * device, of one key size: key_len 16, 24 or 32.  No call reads a master back.  THE TABLE HOLDS MASTER KEYS: PROTECT IT LIKE KEYS.
 * THE DERIVATION (RFC 3711 4.3.1; RFC 6188 for AES-192 / AES-256 master keys; labels as RFC 7714 11 uses them): with the master key mk, the 14-byte master salt ms, a
 * label byte and the 48-bit r = index DIV key_derivation_rate (0 where the rate is 0),
 *   x = ms XOR (0^56 | label | be48(r)), 14 bytes: the label XORs into byte 7, r into bytes 8 .. 13;
 *   output = E_mk(x | be16(0)) | E_mk(x | be16(1)) | ..., truncated.
 * Labels: SRTP key 0x00, SRTP salt 0x02, SRTCP key 0x03, SRTCP salt 0x05; the GCM transforms have no authentication key.  The session key is key_len bytes (two blocks
 * for AES-192 / AES-256), the session salt the first 12 bytes of its block -- what aesgcm_keytab_set_tls_iv holds and aesgcm_keytab_srtp_crypt_dev reads.  The PRF's AES
 * size is the master key's, which must be the key table's: AES_128_CM for 16-byte slots, AES_192_CM / AES_256_CM (RFC 6188) otherwise.
 * THE MASTER SALT IS 14 BYTES HERE, ALWAYS.  The AEAD profiles of RFC 7714 carry a 12-byte master salt; as this library reads RFC 7714 11, the PRF takes it multiplied
 * by 2^16, that is, WITH TWO ZERO BYTES APPENDED on the right: a caller with a 12-byte salt passes those 14 bytes (the Python binding pads).
 *   aesgcm_srtp_kdf_create   every record unset.  AESGCM_EARG for a key_len other than 16 / 24 / 32, n_masters == 0 or >= 2^31.
 *   aesgcm_srtp_kdf_set      HOST master keys (n * key_len bytes) and salts (n * 14 bytes) into records first .. first + n - 1, through the table's staging buffer on
 *                            `stream`, zeroed behind the copy; the library's host copy is wiped before the call returns (as aesgcm_kdf_set).
 *   aesgcm_srtp_kdf_set_dev  n master keys and salts from DEVICE memory (n * key_len and n * 14 bytes, no alignment asked) into the records d_idx[i]; an index out
 *                            of range is refused.
 *   aesgcm_srtp_kdf_clear    records first .. first + n - 1 zeroed and unset.
 *   aesgcm_srtp_kdf_status   as aesgcm_keytab_status: the LOWEST entry index an install or set_dev call refused since the last read, which clears it.
 *   aesgcm_srtp_kdf_destroy  waits for the device, zeroes the records and the staging buffer, frees.
 * INSTALL: aesgcm_srtp_kdf_install_dev(k, kind, keytab, n, d_idx, d_slots, d_r, stream), kind = AESGCM_SRTP_RTP or AESGCM_SRTP_RTCP.  For entry i with the master of
 * record d_idx[i] and r = d_r[i] (DEVICE memory, n uint64; d_r = NULL: every r is 0):
 *   slot d_slots[i] of `keytab` becomes exactly what aesgcm_keytab_set_dev makes of the session key under the kind's key label -- round keys, H, its powers, the set
 *   marker -- and its TLS-IV field what aesgcm_keytab_set_tls_iv makes of the first 12 bytes of the session salt under the kind's salt label.
 * An SRTP and an SRTCP slot of one stream are two calls over the same d_idx.  A new key-derivation period is the same call with the new r, into fresh slots where packets
 * of the old period are still in flight (INTEGRATION.md "Key derivation").
 * AESGCM_EARG, before a device is touched: a kind that is neither constant; k or keytab NULL; (n == 0 is AESGCM_OK;) d_idx or d_slots NULL; n >= 2^31; a key table of
 * another device; a key table whose key size is not the master table's.
 * REFUSED ENTRIES are skipped whole -- NOTHING an entry names is written -- when d_idx[i] is out of range, the record is unset or cleared, d_slots[i] is out of range,
 * or d_r[i] >= 2^48.  The lowest such index goes to the MASTER table's status word; the key table's status is not touched.
 * NO DERIVED KEY IN MEMORY: the lane that derives a session key loads the master key into registers, runs its key schedule there, encrypts the counter blocks and runs
 * the session key's schedule from the output words; neither the master key's schedule nor the PRF's output is stored anywhere, a session key and salt nowhere but in
 * the slot's fields.
 * One launch per install, a lane per derived value (k_srtp_kdf_install: entries x {key, salt}); no allocation, no event, no host synchronisation, nothing read back:
 * install is capture-safe (CAPTURE, under "key tables" above) and asynchronous on `stream`.  Ordering and thread safety as aesgcm_kdf_*.
 * OUT OF SCOPE: the DTLS-SRTP exporter (not this table's: aesgcm_prf12_export_srtp_dev below fills these records on the device) and SDES; the authentication-key labels (0x01, 0x04) and the AES-CM / HMAC-SHA1 transforms they serve; RFC 6904's header
 * labels; counting packets to the next period (r is the caller's, per entry); the TLS 1.2 / DTLS 1.2 PRF (not this table's: aesgcm_prf12_* under "TLS 1.2 PRF" below); IKEv2's prf+ (not this table's: aesgcm_prfplus_* under "IKEv2 PRF+" below). */
typedef struct aesgcm_srtp_kdf aesgcm_srtp_kdf;
AESGCM_API int aesgcm_srtp_kdf_create(aesgcm_srtp_kdf **out, int device, size_t key_len, size_t n_masters);
AESGCM_API int aesgcm_srtp_kdf_set(aesgcm_srtp_kdf *k, size_t first, size_t n, const uint8_t *keys, const uint8_t *salts, void *stream);
AESGCM_API int aesgcm_srtp_kdf_set_dev(aesgcm_srtp_kdf *k, size_t n, const uint32_t *d_idx, const void *d_keys, const void *d_salts, void *stream);
AESGCM_API int aesgcm_srtp_kdf_clear(aesgcm_srtp_kdf *k, size_t first, size_t n, void *stream);
AESGCM_API int aesgcm_srtp_kdf_install_dev(aesgcm_srtp_kdf *k, uint32_t kind, aesgcm_keytab *keytab, size_t n, const uint32_t *d_idx, const uint32_t *d_slots,
                                const uint64_t *d_r, void *stream);
AESGCM_API int aesgcm_srtp_kdf_status(aesgcm_srtp_kdf *k, int *code, uint64_t *detail);
AESGCM_API int aesgcm_srtp_kdf_destroy(aesgcm_srtp_kdf *k);

/* ---------------------------------------------------------------- TLS 1.2 PRF: TLS 1.2 and DTLS 1.2 AES-GCM keys, and DTLS-SRTP master keys, from master secrets that never leave the device
 * In TLS 1.2 and DTLS 1.2 every key of a connection comes from its 48-byte master secret and the two hello randoms by the PRF of RFC 5246 section 5:
 *   PRF(secret, label, seed) = P_hash(secret, label | seed) = T(1) | T(2) | ..., A(0) = label | seed, A(j) = HMAC(secret, A(j - 1)), T(j) = HMAC(secret, A(j) | label | seed),
 * over HMAC-SHA-256, or HMAC-SHA-384 for the suites that name SHA384.  aesgcm_prf12 is a table of n_masters records on the device, each a master secret and its
 * connection's client random and server random (32 bytes each), of one PRF hash: hash_len 32 = SHA-256, 48 = SHA-384.  No call reads a record back.  THE TABLE HOLDS
 * MASTER SECRETS: PROTECT IT LIKE KEYS -- whoever holds a master secret holds every key of its connection, and of every connection resumed from its session.
 *   aesgcm_prf12_create    every record unset.  AESGCM_EARG for a hash_len other than 32 / 48, n_masters == 0 or >= 2^31.
 *   aesgcm_prf12_set       HOST master secrets (n * 48 bytes), client randoms and server randoms (n * 32 bytes each) into records first .. first + n - 1, through the
 *                          table's staging buffer on `stream`, zeroed behind the copy; the library's host copy is wiped before the call returns (as aesgcm_kdf_set).
 *   aesgcm_prf12_set_dev   n masters and randoms from DEVICE memory (n * 48, n * 32 and n * 32 bytes, no alignment asked) into the records d_idx[i]; an index out of
 *                          range is refused.
 *   aesgcm_prf12_clear     records first .. first + n - 1 zeroed and unset.
 *   aesgcm_prf12_status    as aesgcm_keytab_status: the LOWEST entry index an install, export or set_dev call refused since the last read, which clears it.
 *   aesgcm_prf12_destroy   waits for the device, zeroes the records and the staging buffer, frees.
 * INSTALL: aesgcm_prf12_install_dev(p, keytab, n, d_idx, d_client_slots, d_server_slots, stream).  For entry i with the record d_idx[i]:
 *   key_block = P_hash(master, "key expansion" | server_random | client_random) = client_write_key | server_write_key | client_write_IV[4] | server_write_IV[4], the keys
 *   of the key table's key_len (RFC 5246 6.3; RFC 5288 3: an AEAD suite has no MAC keys, and its fixed IV is four bytes);
 *   slot d_client_slots[i] of `keytab` becomes exactly what aesgcm_keytab_set_dev makes of client_write_key -- round keys, H, its powers, the set marker -- and its
 *   TLS-IV field what aesgcm_keytab_set_tls_iv makes of client_write_IV | 8 zero bytes: what aesgcm_keytab_records_crypt_dev (TLS 1.2) and aesgcm_keytab_dtls_crypt_dev
 *   (DTLS 1.2) read; slot d_server_slots[i] gets server_write_key and server_write_IV the same way.
 * Either array may be NULL (not both: AESGCM_EARG), and an entry of 0xFFFFFFFF installs nothing for that direction: an endpoint installs its write key into its
 * sending table and the peer's into its receiving one, in two calls or in one.  The table's key size may be 16, 24 or 32 with either hash.  AESGCM_EARG for p or
 * keytab NULL, d_idx NULL, n >= 2^31 and a key table of another device; n == 0 is AESGCM_OK.
 * EXPORT: aesgcm_prf12_export_srtp_dev(p, masters, n, d_idx, d_client_recs, d_server_recs, stream).  For entry i:
 *   out = P_hash(master, "EXTRACTOR-dtls_srtp" | client_random | server_random), 2 * key_len + 24 bytes = client key | server key | client salt[12] | server salt[12]
 *   with the SRTP master table's key_len (RFC 5705 4 without a context; RFC 5764 4.2; the AEAD profiles' 12-byte salts, RFC 7714 12).  THE RANDOMS STAND IN THE
 *   OTHER ORDER than in key expansion;
 *   record d_client_recs[i] of `masters` becomes exactly what aesgcm_srtp_kdf_set_dev makes of the client's key and of its salt with two zero bytes appended (the 14
 *   bytes that table takes, "SRTP KEY DERIVATION" above); record d_server_recs[i] gets the server's.  NULL and 0xFFFFFFFF as install.
 * AESGCM_EARG as install, and for a master table of another device or of key_len 24 (DTLS-SRTP has no AES-192 profile).  From there aesgcm_srtp_kdf_install_dev derives
 * the session keys: master secret -> exporter -> master table -> install -> aesgcm_keytab_srtp_crypt_dev, as launches on one stream (INTEGRATION.md "Key derivation").
 * REFUSED ENTRIES are skipped whole -- NOTHING an entry names is written, in either direction -- when d_idx[i] is out of range, the record is unset or cleared, or a
 * slot / record it names (other than 0xFFFFFFFF) is out of range.  The lowest such index goes to THIS table's status word; the key table's and the SRTP master
 * table's status words are not touched.
 * THE BOUND: both labels are shorter than 20 bytes, so the seed is at most 84 bytes and every HMAC has a block count that no datum changes (csrc/aesgcm_prf12.h); the
 * ipad and opad states of the master secret are computed once per lane.  A lane computes only as many T(j) as cover the bytes it takes.
 * NO DERIVED KEY IN MEMORY: a derived key, IV or salt is stored nowhere but in the slot's fields or the SRTP master record.  The lane that derives a key runs the key
 * schedule itself, from its registers.
 * One launch per call, a lane per derived value (k_prf12_install: entries x {client key, server key, client IV, server IV}; k_prf12_export: entries x {client,
 * server}); no allocation, no event, no host synchronisation, nothing read back: install and export are capture-safe (CAPTURE, under "key tables" above) and
 * asynchronous on `stream`.  Ordering and thread safety as aesgcm_kdf_*.
 * OUT OF SCOPE: deriving the master secret itself from the premaster secret, with or without the extended master secret of RFC 7627 (the master secret is the
 * caller's); verify_data; the MAC keys of CBC suites (only AEAD key blocks are cut); exporters with a context or other labels; IKEv2's prf+ (not this table's: aesgcm_prfplus_* below) and MACsec's MKA KDF (AES-CMAC, not this table's either: aesgcm_mka_* under "MACSEC MKA" below). */
typedef struct aesgcm_prf12 aesgcm_prf12;
AESGCM_API int aesgcm_prf12_create(aesgcm_prf12 **out, int device, size_t hash_len, size_t n_masters);
AESGCM_API int aesgcm_prf12_set(aesgcm_prf12 *p, size_t first, size_t n, const uint8_t *masters, const uint8_t *client_randoms, const uint8_t *server_randoms, void *stream);
AESGCM_API int aesgcm_prf12_set_dev(aesgcm_prf12 *p, size_t n, const uint32_t *d_idx, const void *d_masters, const void *d_client_randoms, const void *d_server_randoms,
                             void *stream);
AESGCM_API int aesgcm_prf12_clear(aesgcm_prf12 *p, size_t first, size_t n, void *stream);
AESGCM_API int aesgcm_prf12_install_dev(aesgcm_prf12 *p, aesgcm_keytab *keytab, size_t n, const uint32_t *d_idx, const uint32_t *d_client_slots,
                                 const uint32_t *d_server_slots, void *stream);
AESGCM_API int aesgcm_prf12_export_srtp_dev(aesgcm_prf12 *p, aesgcm_srtp_kdf *masters, size_t n, const uint32_t *d_idx, const uint32_t *d_client_recs,
                                     const uint32_t *d_server_recs, void *stream);
AESGCM_API int aesgcm_prf12_status(aesgcm_prf12 *p, int *code, uint64_t *detail);
AESGCM_API int aesgcm_prf12_destroy(aesgcm_prf12 *p);

/* ---------------------------------------------------------------- IKEv2 PRF+: ESP keys of Child SAs from SK_d values that never leave the device
 * An IKEv2 gateway holds one SK_d per IKE SA and cuts the keys of every Child SA from it, at creation and again at every rekey (RFC 7296 2.17):
 *   KEYMAT = prf+(SK_d, Ni | Nr), or prf+(SK_d, g^ir (new) | Ni | Nr) where the exchange carried a Diffie-Hellman (PFS),
 * with prf+ of RFC 7296 2.13:
 *   prf+(K, S) = T1 | T2 | ...,   T1 = prf(K, S | 0x01),   Tn = prf(K, T(n-1) | S | n)   (n one byte),
 * and prf = HMAC-SHA-256, HMAC-SHA-384 or HMAC-SHA-512 (PRF_HMAC_SHA2_256 / _384 / _512, RFC 4868).  aesgcm_prfplus is a table of n_keys SK_d values on the device, of
 * one prf: hash_len 32, 48 or 64, which is also SK_d's length (the prf's preferred key length).  No call reads a record back.  THE TABLE HOLDS SK_d VALUES: PROTECT IT
 * LIKE KEYS -- whoever holds an SK_d holds the keys of every Child SA its IKE SA makes without PFS, and those of the IKE SAs rekeyed from it.
 *   aesgcm_prfplus_create    every record unset.  AESGCM_EARG for a hash_len other than 32 / 48 / 64, n_keys == 0 or >= 2^31.
 *   aesgcm_prfplus_set       HOST SK_d values (n * hash_len bytes) into records first .. first + n - 1, through the table's staging buffer on `stream`, zeroed behind
 *                            the copy; the library's host copy is wiped before the call returns (as aesgcm_kdf_set).
 *   aesgcm_prfplus_set_dev   n SK_d values from DEVICE memory (n * hash_len bytes, no alignment asked) into the records d_idx[i]; an index out of range is refused.
 *   aesgcm_prfplus_clear     records first .. first + n - 1 zeroed and unset.
 *   aesgcm_prfplus_status    as aesgcm_keytab_status: the LOWEST entry index an install or set_dev call refused since the last read, which clears it.
 *   aesgcm_prfplus_destroy   waits for the device, zeroes the records and the staging buffer, frees.
 * INSTALL: aesgcm_prfplus_install_dev(p, keytab, n, d_idx, d_seed, d_seed_off, d_i2r_slots, d_r2i_slots, stream).  For entry i with the SK_d of record d_idx[i]:
 *   THE SEED S is the bytes [d_seed_off[i], d_seed_off[i + 1]) of d_seed (DEVICE memory; d_seed_off: n + 1 uint32 byte offsets): byte-packed, at any alignment, 1 ..
 *   2048 bytes (g^ir of MODP-8192 and two 256-byte nonces).  The seeds are the caller's, per entry, and not the table's: many Child SAs share one IKE SA's SK_d and each
 *   has its own Ni | Nr, so many entries of one call may name the same d_idx, and a rekey is a new seed, not a new record.  WITH PFS THE SEED HOLDS THE DIFFIE-HELLMAN
 *   SHARED SECRET: the buffer is then the caller's to protect and to wipe;
 *   KEYMAT = prf+(SK_d, S) = key_i2r | salt_i2r[4] | key_r2i | salt_r2i[4] (RFC 7296 2.17: the initiator-to-responder SA first; RFC 4106 8.1: within an SA the key, then
 *   its four salt bytes), the keys of the key table's key_len, 16, 24 or 32, with any of the three hashes: direction d's bytes start at d * (key_len + 4);
 *   slot d_i2r_slots[i] of `keytab` becomes exactly what aesgcm_keytab_set_dev makes of key_i2r -- round keys, H, its powers, nr, the set marker -- and its 8-byte salt
 *   field what aesgcm_keytab_set_salt makes of salt_i2r | 00 00 00 00: what the ESP format {8, 16, 8, 4, tag, 0} reads, with or without ESN; xpn and the TLS-IV field
 *   are left alone.  Slot d_r2i_slots[i] gets key_r2i and salt_r2i the same way.  AES-GMAC ESP (ENCR_NULL_AUTH_AES_GMAC, RFC 4543) takes the same KEYMAT.
 * Either slot array may be NULL (not both: AESGCM_EARG), and an entry of 0xFFFFFFFF installs nothing for that direction: an endpoint installs its outbound SA into its
 * sending table and its inbound SA into its receiving one, in two calls or in one.  AESGCM_EARG, before a device is touched, for p or keytab NULL, d_idx, d_seed or
 * d_seed_off NULL, n >= 2^31 and a key table of another device; n == 0 is AESGCM_OK and looks at nothing.
 * REFUSED ENTRIES are skipped whole -- NOTHING an entry names is written, in either direction -- when d_idx[i] is out of range, the record is unset or cleared, a slot
 * it names (other than 0xFFFFFFFF) is out of range, or its seed's offsets fall, or the seed is empty or longer than 2048 bytes.  The lowest such index goes to THIS
 * table's status word; the key table's status word is not touched.
 * NO DERIVED KEY IN MEMORY: a derived key or salt is stored nowhere but in the slot's fields, no T(n) anywhere.  The lane that derives a key runs the key schedule
 * itself, from its registers.
 * One launch per call, a lane per direction (k_prfp_install: entries x {i2r, r2i}; a lane derives its key and salt together and computes only as many T(n) as cover
 * them); no allocation, no event, no host synchronisation, nothing read back: install is capture-safe (CAPTURE, under "key tables" above) and asynchronous on
 * `stream`.  Ordering and thread safety as aesgcm_kdf_*.  So an ESP rekey runs as launches on one stream: aesgcm_txnum_assign_dev refuses at the limit, install with
 * the new nonces into fresh slots, reset the counter, encrypt (INTEGRATION.md "Key derivation").
 * OUT OF SCOPE: the IKE SA's own keys -- SKEYSEED and the SK_d | SK_ai | SK_ar | SK_ei | SK_er | SK_pi | SK_pr split (SK_d is the caller's); IKEv1; PRF_HMAC_SHA1,
 * AES-XCBC and AES-CMAC as prf; ENCR suites with a separate integrity key (only AEAD KEYMAT is cut); MACsec's MKA KDF (AES-CMAC in counter mode; not this table's: aesgcm_mka_* under "MACSEC MKA" below). */
typedef struct aesgcm_prfplus aesgcm_prfplus;
AESGCM_API int aesgcm_prfplus_create(aesgcm_prfplus **out, int device, size_t hash_len, size_t n_keys);
AESGCM_API int aesgcm_prfplus_set(aesgcm_prfplus *p, size_t first, size_t n, const uint8_t *keys, void *stream);
AESGCM_API int aesgcm_prfplus_set_dev(aesgcm_prfplus *p, size_t n, const uint32_t *d_idx, const void *d_keys, void *stream);
AESGCM_API int aesgcm_prfplus_clear(aesgcm_prfplus *p, size_t first, size_t n, void *stream);
AESGCM_API int aesgcm_prfplus_install_dev(aesgcm_prfplus *p, aesgcm_keytab *keytab, size_t n, const uint32_t *d_idx, const void *d_seed, const uint32_t *d_seed_off,
                                   const uint32_t *d_i2r_slots, const uint32_t *d_r2i_slots, void *stream);
AESGCM_API int aesgcm_prfplus_status(aesgcm_prfplus *p, int *code, uint64_t *detail);
AESGCM_API int aesgcm_prfplus_destroy(aesgcm_prfplus *p);

/* ---------------------------------------------------------------- MACSEC MKA: SAKs from CAKs that never leave the device, by the AES-CMAC KDF and AES Key Wrap
 * MKA (IEEE 802.1X-2010 6.2, 9.3, 9.8) keys a MACsec connectivity association from its CAK.  The KEY SERVER derives the SAK, uses it, and distributes it to the peers
 * wrapped by AES Key Wrap (RFC 3394) under the KEK; EVERY OTHER STATION derives the same KEK and unwraps the SAK it received.  A switch plays both roles.
 *   PRF = AES-CMAC (RFC 4493; SP 800-38B) with a 16- or 32-byte key, 16 bytes of output
 *   KDF(Key, Label, Context, Length) = first Length bits of  PRF(Key, 0x01 | Label | 0x00 | Context | be16(Length)) | PRF(Key, 0x02 | ...) | ...
 *   KEK = KDF(CAK, "IEEE8021 KEK", Keyid, 8 * cak_len)      Keyid = the first 16 bytes of the CKN, zero-padded on the right where it is shorter
 *   SAK = KDF(CAK, "IEEE8021 SAK", KS-nonce | MI-value list | KN, 8 * key_len)
 * The counter is one byte; Length is in bits, two bytes, big-endian; both labels are 12 bytes without a terminator (the 0x00 that follows is the formula's).  The KEK has
 * the CAK's length, the SAK the key table's: a 16-byte CAK may produce a 32-byte SAK (two iterations), and the other way round.  The wrapped SAK is RFC 3394 2.2.1 with
 * the default initial value A6A6A6A6A6A6A6A6: key_len + 8 bytes, so 24 or 40.  aesgcm_mka is a table of n_caks CAKs on the device, of one cak_len (16 or 32), each with
 * its 16-byte Keyid.  No call reads a record back.  THE TABLE HOLDS CAKs: PROTECT IT
 * LIKE KEYS -- whoever holds a CAK derives the KEK, unwraps every SAK its association distributes, and may act as its key server.
 *   aesgcm_mka_create        every record unset.  AESGCM_EARG for a cak_len other than 16 / 32, n_caks == 0 or >= 2^31.
 *   aesgcm_mka_set           HOST CAKs (n * cak_len bytes) and Keyids (n * 16 bytes) into records first .. first + n - 1, through the table's staging buffer on `stream`,
 *                            zeroed behind the copy; the library's host copy is wiped before the call returns (as aesgcm_kdf_set).
 *   aesgcm_mka_set_dev       n CAKs and Keyids from DEVICE memory (n * cak_len and n * 16 bytes, no alignment asked) into the records d_idx[i]; an index out of range
 *                            is refused.
 *   aesgcm_mka_clear         records first .. first + n - 1 zeroed and unset.
 *   aesgcm_mka_status        as aesgcm_keytab_status: the LOWEST entry index an install, unwrap or set_dev call refused since the last read, which clears it.
 *   aesgcm_mka_destroy       waits for the device, zeroes the records and the staging buffer, frees.
 * INSTALL (the key server): aesgcm_mka_install_dev(m, keytab, n, d_idx, d_ctx, d_ctx_off, d_slots, d_wrapped, stream).  For entry i with the CAK of record d_idx[i]:
 *   THE CONTEXT is the bytes [d_ctx_off[i], d_ctx_off[i + 1]) of d_ctx (DEVICE memory; d_ctx_off: n + 1 uint32 byte offsets): byte-packed, at any alignment, 1 .. 2048
 *   bytes.  The caller assembles KS-nonce | MI list | be32(KN); the library does not parse it;
 *   slot d_slots[i] of `keytab` (key_len 16 or 32) becomes exactly what aesgcm_keytab_set_dev makes of the SAK -- round keys, H, its powers, nr, the set marker.  The
 *   salt, xpn and TLS-IV fields are left alone: the SCI goes in by aesgcm_keytab_set_salt, the XPN salt by aesgcm_keytab_set_xpn, and both are the caller's;
 *   if d_wrapped is not NULL, entry i's key_len + 8 wrapped bytes go to d_wrapped + i * (key_len + 8) (no alignment asked): what the MKPDU's Distributed SAK parameter
 *   set carries.  A refused entry's bytes there are not written.
 * Many entries may name one record: one SAK serves several SCs, so several slots are several entries.
 * UNWRAP (any other station): aesgcm_mka_unwrap_dev(m, keytab, n, d_idx, d_wrapped, d_slots, d_verdict, stream).  The KEK is derived from record d_idx[i] and unwraps
 *   the key_len + 8 bytes at d_wrapped + i * (key_len + 8) (RFC 3394 2.2.2).  If all eight bytes of the recovered A equal the default initial value, slot d_slots[i] is
 *   built as above; if not, the entry is refused.  Where d_verdict is not NULL, entry i's byte there becomes 0 (installed), 1 (refused for what it names) or 2 (the
 *   integrity check failed).
 * AESGCM_EARG, before a device is touched, for m or keytab NULL, d_idx, d_ctx, d_ctx_off, d_slots (install) or d_idx, d_wrapped, d_slots (unwrap) NULL, n >= 2^31, a key
 * table of another device and a key table of key size 24 (MACsec has no AES-192); n == 0 is AESGCM_OK and looks at nothing.
 * REFUSED ENTRIES are skipped whole -- NOTHING an entry names is written; the verdict byte, where one was asked for, is the only byte a refused entry gets -- when
 * d_idx[i] is out of range, the record is unset or cleared, the slot is out of range, the context's offsets fall, or the context is empty or longer than 2048 bytes, or
 * the unwrap check fails.  The lowest such index goes to THIS table's status word; the key table's status word is not touched.
 * NO DERIVED KEY IN MEMORY: neither the CAK's schedule, the KEK, its schedule, a CMAC subkey nor an unwrapped candidate is stored anywhere; the SAK goes nowhere but
 * the slot's fields.  The lane that derives a key runs the key schedule itself, from its registers.  The wrapped SAK is public and goes to the caller's buffer.
 * One launch per call, a lane per entry (k_mka_install: the same lane derives the SAK and, where asked, the KEK and the wrap; k_mka_unwrap: KEK, the inverse cipher,
 * the check, the slot); no scratch memory, no allocation, no event, no host synchronisation, nothing read back: install and unwrap are capture-safe (CAPTURE, under
 * "key tables" above) and asynchronous on `stream`.  Ordering and thread safety as aesgcm_kdf_*.  So a MACsec rekey runs as launches on one stream:
 * aesgcm_txnum_assign_dev refuses at PN exhaustion, install with KN + 1 into the next AN's slot, set_salt, reset the counter, encrypt; the peer runs unwrap, then its
 * receive windows (INTEGRATION.md "Key derivation").
 * OUT OF SCOPE: CAK and CKN from an EAP MSK ("IEEE8021 EAP CAK" / "IEEE8021 EAP CKN"); the ICK and the ICV of MKPDUs; building or parsing MKPDUs, the KS-nonce's
 * randomness, MI and KN bookkeeping; the XPN salt from MI and KN (the caller's aesgcm_keytab_set_xpn does it: no text of 802.1AEbw is on hand to pin its byte order);
 * AES-192; key wrap with padding (RFC 5649). */
typedef struct aesgcm_mka aesgcm_mka;
AESGCM_API int aesgcm_mka_create(aesgcm_mka **out, int device, size_t cak_len, size_t n_caks);
AESGCM_API int aesgcm_mka_set(aesgcm_mka *m, size_t first, size_t n, const uint8_t *caks, const uint8_t *keyids, void *stream);
AESGCM_API int aesgcm_mka_set_dev(aesgcm_mka *m, size_t n, const uint32_t *d_idx, const void *d_caks, const void *d_keyids, void *stream);
AESGCM_API int aesgcm_mka_clear(aesgcm_mka *m, size_t first, size_t n, void *stream);
AESGCM_API int aesgcm_mka_install_dev(aesgcm_mka *m, aesgcm_keytab *keytab, size_t n, const uint32_t *d_idx, const void *d_ctx, const uint32_t *d_ctx_off,
                               const uint32_t *d_slots, void *d_wrapped, void *stream);
AESGCM_API int aesgcm_mka_unwrap_dev(aesgcm_mka *m, aesgcm_keytab *keytab, size_t n, const uint32_t *d_idx, const void *d_wrapped, const uint32_t *d_slots,
                              uint8_t *d_verdict, void *stream);
AESGCM_API int aesgcm_mka_status(aesgcm_mka *m, int *code, uint64_t *detail);
AESGCM_API int aesgcm_mka_destroy(aesgcm_mka *m);

/* ---------------------------------------------------------------- SSH KEY DERIVATION: AES-GCM keys and initial IVs from K and H that never leave the device (RFC 4253 7.2)
 * An SSH key exchange ends with a shared secret K and an exchange hash H; the first H of a connection is its session identifier.  RFC 4253 7.2 derives
 *   initial IV client to server   = HASH(K | H | "A" | session_id)        encryption key client to server = HASH(K | H | "C" | session_id)
 *   initial IV server to client   = HASH(K | H | "B" | session_id)        encryption key server to client = HASH(K | H | "D" | session_id)
 * each cut to the length needed, HASH the key exchange's own: SHA-256, SHA-384 or SHA-512.  It is a PLAIN HASH, no HMAC.  ("E" / "F", the integrity keys, have no use
 * under AES-GCM.)  aesgcm_sshkdf is a table of n_recs records on the device, of one hash_len (32 / 48 / 64), each
 *   secret = K_enc | H         1 .. max_secret_len bytes (max_secret_len <= 2048, fixed at create).  K_enc is K EXACTLY AS THE KEY EXCHANGE ENCODES IT INTO THE HASH: an
 *                              mpint with its four length bytes (the DH and ECDH exchanges), or a string with its four length bytes (the hybrid exchanges such as
 *                              sntrup761x25519-sha512 and mlkem768x25519-sha256).  The caller says which by passing the bytes; the library does not parse them.
 *   session_id[hash_len]
 * No call reads a record back.  THE TABLE HOLDS KEY-EXCHANGE SECRETS: PROTECT IT LIKE KEYS -- whoever holds K and H derives every key of the connection.
 *   aesgcm_sshkdf_create     every record unset.  AESGCM_EARG for a hash_len other than 32 / 48 / 64, max_secret_len == 0 or > 2048, n_recs == 0 or >= 2^31.
 *   aesgcm_sshkdf_set        HOST secrets (byte-packed: record first + i takes bytes [secret_off[i], secret_off[i + 1]) of `secrets`; secret_off: n + 1 uint32 in HOST
 *                            memory) and session identifiers (n * hash_len bytes) into records first .. first + n - 1, through the table's staging buffer on `stream`,
 *                            zeroed behind the copy; the library's host copy is wiped before the call returns (as aesgcm_kdf_set).  AESGCM_EARG, and nothing stored,
 *                            where offsets fall or a secret is empty or longer than max_secret_len.
 *   aesgcm_sshkdf_set_dev    the same from DEVICE memory (d_secret_off: n + 1 uint32; no alignment asked) into the records d_idx[i]; an index out of range, falling
 *                            offsets, an empty secret or one longer than max_secret_len is refused.
 *   aesgcm_sshkdf_clear      records first .. first + n - 1 zeroed and unset.
 *   aesgcm_sshkdf_status     as aesgcm_keytab_status: the LOWEST entry index an install or set_dev call refused since the last read, which clears it.
 *   aesgcm_sshkdf_destroy    waits for the device, zeroes the records and the staging buffer, frees.
 * INSTALL: aesgcm_sshkdf_install_dev(s, keytab, n, d_idx, d_c2s_slots, d_s2c_slots, stream).  For entry i with record d_idx[i], slot d_c2s_slots[i] of `keytab` becomes
 * exactly what aesgcm_keytab_set_dev makes of the "C" key's first key_len bytes and aesgcm_keytab_set_tls_iv of the "A" value's first 12 -- round keys, H, its powers,
 * nr, the set marker, the IV field -- which is what aesgcm_keytab_ssh_crypt_dev reads; slot d_s2c_slots[i] the same of "D" and "B".  Either array may be NULL (not
 * both); an entry 0xFFFFFFFF installs nothing for that direction.  key_len is the key table's, 16 / 24 / 32 <= hash_len: RFC 4253's extension K2 = HASH(K | H | K1),
 * for values longer than the digest, is NEVER NEEDED AND NOT BUILT.
 * A RE-EXCHANGE (RFC 4253 9) is a set of the new K | H with the SAME session_id, then an install into fresh slots; d_seq starts at 0 under the new key.
 * AESGCM_EARG, before a device is touched, for s or keytab NULL, d_idx NULL, both slot arrays NULL, n >= 2^31, a key table of another device; n == 0 is AESGCM_OK and
 * looks at nothing.
 * REFUSED ENTRIES are skipped whole -- NOTHING an entry names is written -- when d_idx[i] is out of range, the record is unset or cleared, or a slot is out of range.
 * The lowest such index goes to THIS table's status word; the key table's status word is not touched.
 * NO DERIVED KEY IN MEMORY: the lane that derives a key runs the key schedule itself, from its registers; the key goes nowhere but the slot's fields.
 * One launch per call, a lane per entry and letter (k_sshk_install); no scratch memory, no allocation, no event, no host synchronisation, nothing read back: install is
 * capture-safe (CAPTURE, under "key tables" above) and asynchronous on `stream`.  Ordering and thread safety as aesgcm_kdf_*.
 * OUT OF SCOPE: the key exchange itself and the computation of H; RFC 4253's key extension; the integrity keys; chacha20-poly1305@openssh.com's 64-byte keys. */
typedef struct aesgcm_sshkdf aesgcm_sshkdf;
AESGCM_API int aesgcm_sshkdf_create(aesgcm_sshkdf **out, int device, size_t hash_len, size_t max_secret_len, size_t n_recs);
AESGCM_API int aesgcm_sshkdf_set(aesgcm_sshkdf *s, size_t first, size_t n, const uint8_t *secrets, const uint32_t *secret_off, const uint8_t *session_ids, void *stream);
AESGCM_API int aesgcm_sshkdf_set_dev(aesgcm_sshkdf *s, size_t n, const uint32_t *d_idx, const void *d_secrets, const uint32_t *d_secret_off, const void *d_session_ids,
                              void *stream);
AESGCM_API int aesgcm_sshkdf_clear(aesgcm_sshkdf *s, size_t first, size_t n, void *stream);
AESGCM_API int aesgcm_sshkdf_install_dev(aesgcm_sshkdf *s, aesgcm_keytab *keytab, size_t n, const uint32_t *d_idx, const uint32_t *d_c2s_slots,
                                  const uint32_t *d_s2c_slots, void *stream);
AESGCM_API int aesgcm_sshkdf_status(aesgcm_sshkdf *s, int *code, uint64_t *detail);
AESGCM_API int aesgcm_sshkdf_destroy(aesgcm_sshkdf *s);

/* ---------------------------------------------------------------- streaming (beat-by-beat) interface
 * Mirrors the call order the reference harness drives its model with (tb/gcm_test.py:76-85 ->
 * tb/gcm_model.py:21-35): all AAD first, then data; every chunk except the last of its kind must be
 * a multiple of 16 bytes (the harness sends 16-byte beats, tb/gcm_sequencer.py:129-140).  Output for a
 * chunk is complete when the call returns.  State (running GHASH value, block counter) lives on the
 * device between calls, and can be exported and imported (below). */
AESGCM_API int aesgcm_stream_begin(aesgcm_ctx *ctx, const uint8_t iv[12], int decrypt);
AESGCM_API int aesgcm_stream_aad(aesgcm_ctx *ctx, const uint8_t *aad, size_t len);
AESGCM_API int aesgcm_stream_update(aesgcm_ctx *ctx, const uint8_t *in, size_t len, uint8_t *out);
AESGCM_API int aesgcm_stream_final(aesgcm_ctx *ctx, uint8_t tag[16]);
/* The same step on DEVICE pointers (round 6): d_in / d_out 16-byte aligned, may alias; asynchronous on `stream` (NULL = the context's own).  The steps of one session
 * may come on different streams: the library orders them itself (each step's stream waits on the device for the session's previous step; no host synchronisation).  A chunk of any size takes the launch structure a shard of that size takes, so a message of unknown total length that is
 * already on the GPU runs at the rate of aesgcm_shard_crypt_dev.  Every chunk but the last a multiple of 16 bytes.  As a shard, a chunk reads exactly `len` bytes of d_in and
 * writes exactly `len` bytes of d_out: no slack behind the ragged last chunk, and chunks may go to buffers that touch. */
AESGCM_API int aesgcm_stream_update_dev(aesgcm_ctx *ctx, const void *d_in, size_t len, void *d_out, void *stream);
/* The state of the open session as 64 bytes the caller can keep, move and pick up again -- in another context of the same key, on another device, in another process
 * (SURVEY.md 5 "checkpoint / resume", 8(f2)): what the RTL holds in its Y register (src/gcm_ghash.vhd:174-186) and its counter (src/aes_icb.vhd:97-100) and cannot hand out.
 * blob: version, direction, IV, AAD and data bytes so far, GHASH blocks so far, the running GHASH value (in the library's form: the RTL's Y divided by H), a four-byte key
 * check (E_K of a constant block) and a sum check (not cryptographic).  No key and no table is in the blob, but it is EQUIVALENT TO THE AUTHENTICATION KEY H: the
 * running GHASH value together with the public AAD or ciphertext gives H (after two blocks X0, X1 it is X0 H ^ X1), and H forges tags under this key.  Protect the blob
 * like the key.  aesgcm_stream_export waits for everything the session has enqueued (on the context's stream and on any stream a chunk came on; no device-wide
 * synchronisation) and leaves the session open; aesgcm_stream_import opens a session in `ctx` at exactly that point (AESGCM_ESTATE if one is open already; AESGCM_EARG for
 * a blob that is damaged, of another version, exported under another key, or whose fields disagree -- e.g. the ragged bit and the lengths), after which aesgcm_stream_aad / _update / _update_dev / _final go on as if nothing had happened. */
#define AESGCM_STREAM_STATE_BYTES 64
AESGCM_API int aesgcm_stream_export(aesgcm_ctx *ctx, uint8_t blob[AESGCM_STREAM_STATE_BYTES]);
AESGCM_API int aesgcm_stream_import(aesgcm_ctx *ctx, const uint8_t blob[AESGCM_STREAM_STATE_BYTES]);

/* ---------------------------------------------------------------- whole messages, host pointers, pipelined
 * For data that does not start on the GPU: the message is cut into chunk_bytes
 * pieces (0 = 64 MiB); H2D of chunk k+1, the fused kernel on chunk k and D2H of chunk k-1 overlap on three
 * HIP streams, and the running GHASH value is carried between chunks on the device (state the RTL and the
 * pycryptodome model cannot export).  Results are bit-identical to aesgcm_encrypt/aesgcm_decrypt.  Buffers from
 * aesgcm_host_alloc (page-locked) make the copies true DMA; pageable buffers work but copy slower.  The chunk-to-
 * chunk GHASH value uses the context's streaming slot: inside an open aesgcm_stream_begin .. aesgcm_stream_final
 * session these calls return AESGCM_ESTATE. */
AESGCM_API int aesgcm_encrypt_pipelined(aesgcm_ctx *ctx, const uint8_t iv[12], const uint8_t *aad, size_t aad_len,
                             const uint8_t *pt, size_t len, uint8_t *ct, uint8_t tag[16], size_t chunk_bytes);
AESGCM_API int aesgcm_decrypt_pipelined(aesgcm_ctx *ctx, const uint8_t iv[12], const uint8_t *aad, size_t aad_len,
                             const uint8_t *ct, size_t len, uint8_t *pt, const uint8_t *expect_tag, uint8_t tag_out[16],
                             size_t chunk_bytes);
AESGCM_API int aesgcm_host_alloc(void **h_ptr, size_t bytes);
AESGCM_API int aesgcm_host_free(void *h_ptr);

/* ---------------------------------------------------------------- device memory helpers
 * (so that a Python/ctypes host needs no other GPU runtime binding) */
AESGCM_API int aesgcm_dev_alloc(int device, void **d_ptr, size_t bytes);
AESGCM_API int aesgcm_dev_free(int device, void *d_ptr);
AESGCM_API int aesgcm_dev_upload(int device, void *d_dst, const void *h_src, size_t bytes);
AESGCM_API int aesgcm_dev_download(int device, void *h_dst, const void *d_src, size_t bytes);
AESGCM_API int aesgcm_dev_sync(int device);
/* device-to-device copy by a plain 16-bytes-per-lane kernel (asynchronous on `stream`): the measured HBM
 * read+write figure bench.py reports beside the datasheet peak (SURVEY.md 8(d) "measured copy-kernel figure"). */
AESGCM_API int aesgcm_dev_copy(int device, void *d_dst, const void *d_src, size_t bytes, void *stream);
/* SplitMix64 counter-based synthetic stream: little-endian 64-bit word w of stream
 * `seed` for w = first_word ..; bytes [0, len) of the buffer. */
AESGCM_API int aesgcm_fill_splitmix64_dev(int device, void *d_buf, size_t len, uint64_t seed, uint64_t first_word, void *stream);

/* A pair of HIP events: aesgcm_timer_start / _stop record them on `stream` (NULL = the default stream) around whatever the
 * caller enqueues there; aesgcm_timer_ms waits for the second and returns the elapsed device time.  For timing launches
 * of the context-free entry points (bench.py --config cfg5: aesgcm_batch_crypt_dev) on the stream they run on. */
typedef struct aesgcm_timer aesgcm_timer;
AESGCM_API int aesgcm_timer_create(aesgcm_timer **out, int device);
AESGCM_API int aesgcm_timer_start(aesgcm_timer *t, void *stream);
AESGCM_API int aesgcm_timer_stop(aesgcm_timer *t, void *stream);
AESGCM_API int aesgcm_timer_ms(aesgcm_timer *t, double *ms);
AESGCM_API int aesgcm_timer_destroy(aesgcm_timer *t);

/* ---------------------------------------------------------------- measurement support
 * When enabled, every launch of the fused CTR+GHASH kernel on this context is bracketed with HIP
 * events on the stream it is launched on (see aesgcm_ctx_split for split ranges).  aesgcm_ctx_timing_read synchronises those events and
 * returns the number of launches and their summed duration since the last reset. */
AESGCM_API int aesgcm_ctx_timing_enable(aesgcm_ctx *ctx, int on);
AESGCM_API int aesgcm_ctx_timing_read(aesgcm_ctx *ctx, uint64_t *n_launches, double *total_ms, int reset);
/* Per-workgroup trace of the most recent fused-kernel launch made while timing was enabled: for each of
 * the *n_wgs workgroups four uint64 {start, end of its last wave (100 MHz wall clock), HW_ID | XCC_ID << 32,
 * (chunks its waves processed) | (sum over its waves of shader-clock kilocycles resident) << 32}. */
AESGCM_API int aesgcm_ctx_wg_trace(aesgcm_ctx *ctx, uint64_t *out, size_t max_wgs, size_t *n_wgs);
/* Ceiling of the formulation (SURVEY.md 8(d) "measured LDS/VALU ceilings next to the result"): runs the fused kernel's
 * instruction stream over a virtual range of `nbytes` with its global loads and stores removed (no buffer is touched)
 * and returns its duration and the number of 16-byte blocks it covered.  bench.py prints 32 B x blocks / time beside
 * the achieved figure, measured in the same process. */
AESGCM_API int aesgcm_ctx_ceiling_probe(aesgcm_ctx *ctx, size_t nbytes, double *ms, uint64_t *blocks);
/* geometry the context chose (workgroups, lanes per workgroup, LDS bytes per workgroup) */
AESGCM_API int aesgcm_ctx_geometry(const aesgcm_ctx *ctx, int *n_workgroups, int *wg_lanes, int *lds_bytes);
/* the same for k_body, the kernel that runs the aligned middle of ranges >= 256 MiB (four T-tables: one 1024-lane workgroup per CU) */
AESGCM_API int aesgcm_ctx_body_geometry(const aesgcm_ctx *ctx, int *n_workgroups, int *wg_lanes, int *lds_bytes);
/* How a data range of `len` bytes starting at block `first_block` of its message is launched: large ranges are cut
 * into head (k_main), an aligned middle whose counters start at a multiple of 256 (k_body: rounds 1-2 without LDS
 * lookups) and tail (k_main).  *body_blocks = 0 means one k_main launch.  With timing enabled, only the k_body
 * launch of a split range is timed and traced (it is the measured kernel). */
AESGCM_API int aesgcm_ctx_split(const aesgcm_ctx *ctx, size_t len, uint64_t first_block, uint64_t *head_blocks, uint64_t *body_blocks);

#ifdef __cplusplus
}
#endif
#endif /* AESGCM_H */
