// aesgcm_host.hip -- the host runtime of libaesgcm_hip.so: contexts and per-device state, the runner of single messages, the shape rules of the packet paths
// (DESIGN.md section 8), the scratch and the cut of the row path (aesgcm_rows.h), the pipelined host-buffer path.  No device code and no kernel name in this file:
// launches go through the klaunch_* functions of aesgcm_kernels.hip (aesgcm_internal.h).
// Single messages are PLAN, THEN RUN.  Which launches a whole message, a shard, a streaming chunk or aesgcm_ghash takes is decided by
// msg_plan (aesgcm_msgplan.h: no HIP call, no context) from the call, the context's options and the addresses of its scratch -- k_main, k_body dealt or cyclic and
// in which shape, the k_fold levels, who closes the tag, the k_combine launches, each with its finished parameter struct.  msg_run below walks that list on a stream
// and owns everything that touches the runtime, once: growing `parts` to what the plan needs, the trace and the event pair of a timed launch, last_np and
// last_shape, the fused-launch event, the queue sets' toggle behind a dealt launch, a generation number taken for every launch that publishes and given back when
// it fails, the error texts, and the stop at the first step that fails.  The CPU harness walks the same plans with its kernel emulators (tests/host_emul), and
// tests/golden/launch_plan_msg.txt pins them launch by launch (tests/fake_hip/msg_drive.py).
#include "aesgcm_internal.h"
#include "aesgcm_msgplan.h"

#include <algorithm>
#include <new>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

// The one HIP entry point this library can do without: batch_plan asks it whether a call's stream is being captured.  A weak reference, so that the library still loads
// over a HIP runtime that has no stream capture (an older one, a test double); there no stream captures, and batch_plan does not ask.
#pragma weak hipStreamIsCapturing

thread_local char g_err[256] = "";
int hip_fail(hipError_t e, const char *what) {
    snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
    return AESGCM_EHIP;
}

std::mutex &g_mu = *new std::mutex();
std::vector<DeviceState> &g_dev = *new std::vector<DeviceState>();     // never destroyed (as g_ctxs): contexts may outlive this library's static destructors

int device_state(int device, DeviceState **out) {
    std::lock_guard<std::mutex> lk(g_mu);
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) { snprintf(g_err, sizeof g_err, "device %d out of range (%d visible)", device, n); return AESGCM_EHIP; }
    if ((int)g_dev.size() < n) g_dev.resize(n);
    DeviceState &d = g_dev[device];
    if (!d.tables) {
        HIPCHK(hipSetDevice(device));
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, device));
        d.n_cu = prop.multiProcessorCount;
        DevTables *t = nullptr;
        HIPCHK(hipMalloc(&t, sizeof(DevTables)));
        HIPCHK(klaunch_init_tables(t));
        HIPCHK(hipDeviceSynchronize());
        d.tables = t;
        HIPCHK(hipMalloc(&d.batch_counter, 4 * BATCH_DISPENSERS));
        HIPCHK(hipMemset(d.batch_counter, 0, 4 * BATCH_DISPENSERS));
    }
    *out = &d;
    return AESGCM_OK;
}




int set_lds_attrs(int device, DeviceState *ds) {
    // 72 KiB and more of dynamic LDS per workgroup exceed the 64 KiB default cap: opt in once per kernel instance and device (klaunch_set_attributes, in the kernels' translation unit)
    std::lock_guard<std::mutex> lk(g_mu);
    if (ds->attrs) return AESGCM_OK;
    HIPCHK(hipSetDevice(device));
    HIPCHK(klaunch_set_attributes());
    ds->attrs = true;
    return AESGCM_OK;
}


int grow_parts(aesgcm_ctx *c, size_t need) {
    if (need <= c->parts_cap) return AESGCM_OK;
    if (c->parts) { HIPCHK(hipDeviceSynchronize()); HIPCHK(hipFree(c->parts)); c->parts = nullptr; c->parts_cap = 0; }   // rare: first big message
    size_t n = need < 4096 ? 4096 : need;
    hipError_t e = hipMalloc(&c->parts, n * 64 * sizeof(uint4));
    if (e == hipErrorOutOfMemory) return AESGCM_ENOMEM;
    if (e != hipSuccess) return hip_fail(e, "hipMalloc");
    c->parts_cap = n;
    return AESGCM_OK;
}

// ---------------------------------------------------------------- single messages: plan (aesgcm_msgplan.h), then run
bool cyc_capable(const aesgcm_ctx *c) {
#if AESGCM_T4
    return (u32)c->G / 2 * (AESGCM_BODY_WG / 64) == BODY_CYC_WAVES && c->cyc_max_pieces > c->cyc_min_fused;
#else
    return false;
#endif
}
// Is a message of ANOTHER context of this device under way right now?  Every result goes to its context's pinned host slot with the generation number of its
// launch behind it, so "under way" is: the slot does not show the generation last launched.  What the half shape of the cyclic rows is for (two messages
// share every CU); asked once per whole-message launch, a mutex and a few loads.  Contexts register in ctx_create_common and leave in ctx_destroy.
std::vector<aesgcm_ctx *> &g_ctxs = *new std::vector<aesgcm_ctx *>();          // never destroyed: contexts may be destroyed after this library's static destructors have run
bool others_in_flight(const aesgcm_ctx *c) {
    std::lock_guard<std::mutex> lk(g_mu);
    for (const aesgcm_ctx *o : g_ctxs) {
        if (o == c || o->device != c->device || !o->h_tag) continue;
        const u64 launched = __atomic_load_n(&o->tag_gen, __ATOMIC_RELAXED);
        if (__atomic_load_n(reinterpret_cast<const u64 *>(o->h_tag + 1), __ATOMIC_RELAXED) != launched) return true;
    }
    return false;
}

// k_combine on `st`; a result that goes to the tag slot is mirrored to the pinned host slot under a new generation number.  Beside the runner, for the calls whose
// one launch is no message's plan: the tag from a chaining value (aesgcm_stream_final, the pipelined path) and from gathered partials (aesgcm_shard_finalize_*)
int launch_combine(aesgcm_ctx *c, CombineParams p, hipStream_t st) {
    const bool to_slot = p.out == c->d_tag;
    if (to_slot) { p.out_host = c->h_tag_dev; p.gen = gen_take(c); }
    const hipError_t le = klaunch_combine(st, c->km, c->tables, p);
    if (le != hipSuccess) { if (to_slot) gen_give_back(c); return hip_fail(le, "k_combine launch"); }
    return AESGCM_OK;
}
// k_main or k_body as the step says, with the context's timing (trace, event pair) around it when it is the measured launch
static int launch_rows(aesgcm_ctx *c, MsgStep &t, hipStream_t st) {
    const bool main = t.kind == MsgStep::MAIN, timed = c->timing && t.measured;
    u64 **trace = main ? &t.m.trace : &t.b.trace;
    u64 *gen = main ? &t.m.gen : &t.b.gen;
    if (timed) { *trace = c->d_trace; HIPCHK(hipMemsetAsync(c->d_trace, 0, sizeof(u64) * 4 * AESGCM_GMAX, st)); }
    if (t.measured) c->last_np = t.wgs;
    std::pair<hipEvent_t, hipEvent_t> evp;
    if (timed) {
        if (!c->ev_pool.empty()) { evp = c->ev_pool.back(); c->ev_pool.pop_back(); }
        else { HIPCHK(hipEventCreate(&evp.first)); HIPCHK(hipEventCreate(&evp.second)); }
        HIPCHK(hipEventRecord(evp.first, st));
    }
    if (t.publishes) *gen = gen_take(c);
    const hipError_t le = main ? klaunch_main(t.mode, c->nr, t.wgs, st, c->km, c->tables, t.m)
                               : klaunch_body(t.mode, c->nr, t.b.cyc != 0, t.b.cyc && t.b.cw == BODY_CYC_WAVES_HALF, t.wgs, st, c->km, c->tables, t.b);
    if (le != hipSuccess) {                          // nothing ran: the queues were not touched on the device
        if (timed) c->ev_pool.push_back(evp);
        if (t.publishes) gen_give_back(c);
        return hip_fail(le, main ? "k_main launch" : "k_body launch");
    }
    if (t.dealt) c->qset ^= 1u;                       // the launch leaves the other set zeroed for the next dealt one
    if (timed) { HIPCHK(hipEventRecord(evp.second, st)); c->ev.push_back(evp); }
    if (c->ev_fused) HIPCHK(hipEventRecord(c->ev_fused, st));
    return AESGCM_OK;
}
// The launches of a call on `st`: what msg_plan decides, step by step, up to the first that fails.  The plan is made against the context as it stands -- its options,
// its scratch (parts grown first to what the plan needs), the queue set in turn -- and every launch that publishes takes its generation number as it is made.
int msg_run(aesgcm_ctx *c, const MsgCall &call, hipStream_t st) {
    const MsgRules rules = {(u32)c->G, c->tw_override, c->body_min, cyc_capable(c), c->cyc_fuse, c->fold_close, c->cyc_half, c->cyc_prio,
                            c->cyc_min, c->cyc_min_fused, c->cyc_half_max, c->cyc_max, c->cyc_max_fused, c->cyc_max_pieces};
    int in_flight = -1;                               // asked once at most, however often the plan is made
    auto others = [&] { if (in_flight < 0) in_flight = others_in_flight(c); return in_flight != 0; };
    MsgPlan pl;
    for (;;) {
        const MsgScratch s = {c->parts, c->fold_a, c->fold_b, c->d_tag, c->h_tag_dev, {c->d_counter + 16 * 1, c->d_counter + 16 * (1 + AESGCM_NQ)}, c->qset, c->d_cyc,
                              reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(c->km) + offsetof(KeyMaterial, ptab))};
        msg_plan(pl, call, rules, s, others);
        if (pl.parts_need <= c->parts_cap) break;
        const int rc = grow_parts(c, pl.parts_need);
        if (rc) return rc;
    }
    if (call.goal == MSG_TAG) c->last_shape = pl.shape;
    for (u32 k = 0; k < pl.n; k++) {
        MsgStep &t = pl.step[k];
        int rc = AESGCM_OK;
        switch (t.kind) {
        case MsgStep::CLEAR: HIPCHK(hipMemsetAsync(t.clear, 0, 16, st)); break;
        case MsgStep::MAIN: case MsgStep::BODY: rc = launch_rows(c, t, st); break;
        case MsgStep::FOLD: {
            if (t.publishes) t.f.close.gen = gen_take(c);
            const hipError_t le = klaunch_fold(t.wgs, t.publishes, st, c->km, t.f);
            if (le != hipSuccess) { if (t.publishes) gen_give_back(c); rc = hip_fail(le, "k_fold launch"); }
            break;
        }
        case MsgStep::COMBINE: rc = launch_combine(c, t.c, st); break;
        }
        if (rc) return rc;
    }
    if (pl.fold_overflow) snprintf(g_err, sizeof g_err, "k_fold: %u output items do not fit the level's buffer", pl.fold_overflow);
    return pl.rc;
}

int check_lengths(u64 aad_len, u64 len) {
    if (len > MAX_DATA) return AESGCM_ETOOLONG;
    if ((aad_len + 15) / 16 + (len + 15) / 16 >= MAX_SEQ_BLOCKS) return AESGCM_ETOOLONG;
    return AESGCM_OK;
}

// whole message on device pointers; leaves the tag in c->d_tag[0]
int crypt_dev(aesgcm_ctx *c, int dec, const uint8_t iv[12], const void *d_aad, u64 aad_len,
                     const void *d_in, u64 len, void *d_out, hipStream_t st) {
    int rc = check_lengths(aad_len, len);
    if (rc) return rc;
    if (aad_len && !d_aad) return AESGCM_EARG;
    if (len && (!d_in || !d_out)) return AESGCM_EARG;
    HIPCHK(hipSetDevice(c->device));
    return msg_run(c, MsgCall{MSG_TAG, dec ? MODE_DEC : MODE_ENC, iv, d_aad, aad_len, d_in, len, d_out, 0, nullptr, 0, false}, st);
}

// The tag of the last result enqueued for the host slot: the kernel stores it in pinned host memory and then publishes
// the generation number; the host polls that number for a short while (a kernel-completion interrupt costs ~10 us on
// this platform, a poll of coherent host memory well under one) and falls back to a stream synchronisation for long-
// running work or if anything went wrong.
// What has happened when this returns: a tag published from INSIDE a launch (k_body's cyclic rows, cyc_close; k_fold's closing, acc_arrive) is seen while that
// launch is still running, and this function does NOT wait for its end -- the stream is not synchronised.  Every byte of the result is in device memory all the
// same: the rows store through the L2 (global_store ... sc0 sc1, gstore16_wt / gstore*_wt_at, AESGCM_BODY_WT), each workgroup waits for the acknowledgement of
// its own stores (s_waitcnt vmcnt(0)) before it counts itself arrived, and the tag is published by the workgroup that counts the last arrival; the launch
// retires a few microseconds later.  examples/early_read.cpp (tests/test_gpu_cyclic.py) is the standing check: a copy ordered behind nothing reads the whole
// result the moment the tag is there.  Tags that come from k_combine or k_main's tail are published by the last kernel of the call.
int fetch_tag(aesgcm_ctx *c, hipStream_t st, uint8_t tag[16]) {
    const u64 want = gen_now(c);
    const volatile u64 *gen = reinterpret_cast<const volatile u64 *>(c->h_tag + 1);
    if (!poll_gens(gen, 1, 0, want, c->poll_ns)) {                  // poll for at most ~200 us, then block in the runtime
        HIPCHK(hipStreamSynchronize(st));
        // the stream the message was enqueued on has drained: its tag is there -- unless `st` is not that stream, or the launch failed after the number was taken
        if (__atomic_load_n(gen, __ATOMIC_ACQUIRE) != want) {
            snprintf(g_err, sizeof g_err, "the host slot shows generation %llu, not %llu: the stream passed is not the one the message was enqueued on", (unsigned long long)__atomic_load_n(gen, __ATOMIC_ACQUIRE), (unsigned long long)want);
            return AESGCM_ESTATE;
        }
    }
    memcpy(tag, c->h_tag, 16);
    return AESGCM_OK;
}
// The poll of a host slot: up to poll_ns, wait for the n generation words at w, `stride` words apart, to show `gen`; whether all did.  The clock is read every 64th turn.
bool poll_gens(const volatile u64 *w, size_t n, size_t stride, u64 gen, long poll_ns) {
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (u32 spin = 0;; ++spin) {
        size_t m = 0;
        while (m < n && __atomic_load_n(w + m * stride, __ATOMIC_ACQUIRE) == gen) m++;
        if (m == n) return true;
        if ((spin & 63u) == 63u) {
            clock_gettime(CLOCK_MONOTONIC, &t1);
            if ((t1.tv_sec - t0.tv_sec) * 1000000000L + (t1.tv_nsec - t0.tv_nsec) > poll_ns) return false;
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
}

int ct_compare16(const uint8_t *a, const uint8_t *b) {
    unsigned d = 0;
    for (int i = 0; i < 16; i++) d |= (unsigned)(a[i] ^ b[i]);
    return d == 0;
}

int grow(unsigned char **p, size_t *cap, size_t need) {
    if (need <= *cap) return AESGCM_OK;
    if (*p) { hipError_t e = hipFree(*p); *p = nullptr; *cap = 0; if (e != hipSuccess) return hip_fail(e, "hipFree"); }
    size_t n = need < 4096 ? 4096 : need;
    hipError_t e = hipMalloc((void **)p, n);
    if (e == hipErrorOutOfMemory) return AESGCM_ENOMEM;
    if (e != hipSuccess) return hip_fail(e, "hipMalloc");
    *cap = n;
    return AESGCM_OK;
}

// ---------------------------------------------------------------- device tables (aesgcm_internal.h, DevTable)
int devtab_create(DevTable *b, int device, size_t state_bytes, void **state, const char *who) {
    DeviceState *ds;
    int rc = device_state(device, &ds);            // (AESGCM_EHIP without a device)
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    b->device = device;
    hipError_t e = hipMalloc(state, state_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&b->status, sizeof(u32));
    if (e == hipSuccess) e = hipMemset(*state, 0, state_bytes);
    if (e == hipSuccess) e = hipMemset(b->status, 0xFF, sizeof(u32));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        if (*state) (void)hipFree(*state);
        if (b->status) (void)hipFree(b->status);
        *state = nullptr; b->status = nullptr;
        return e == hipErrorOutOfMemory ? AESGCM_ENOMEM : hip_fail(e, who);
    }
    return AESGCM_OK;
}

int devtab_stage(DevTable *b, size_t bytes, hipStream_t st) {
    if (bytes > b->stage_cap) {
        if (b->stage) { HIPCHK(hipFree(b->stage)); b->stage = nullptr; b->stage_cap = 0; }   // hipFree waits for the launches and copies that may still read it
        const hipError_t e = hipMalloc((void **)&b->stage, bytes);
        if (e == hipErrorOutOfMemory) return AESGCM_ENOMEM;
        if (e != hipSuccess) return hip_fail(e, "hipMalloc");
        b->stage_cap = bytes;
    }
    if (!b->stage_done) HIPCHK(hipEventCreateWithFlags(&b->stage_done, hipEventDisableTiming));
    else HIPCHK(hipStreamWaitEvent(st, b->stage_done, 0));
    return AESGCM_OK;
}

int devtab_put(DevTable *b, void *dst, const void *host, size_t bytes, hipStream_t st, bool secret) {
    return devtab_staged(*b, bytes, st, secret, [&]() -> int {
        HIPCHK(hipMemcpyAsync(b->stage, host, bytes, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dst, b->stage, bytes, hipMemcpyDeviceToDevice, st));
        return AESGCM_OK;
    });
}

int devtab_get(DevTable *b, void *host, const void *src, size_t bytes, hipStream_t st) {
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipMemcpyAsync(host, src, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return AESGCM_OK;
}

int devtab_clear(DevTable *b, void *at, size_t bytes, hipStream_t st) {
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipMemsetAsync(at, 0, bytes, st));
    return AESGCM_OK;
}

void host_wipe(void *p, size_t n) { volatile unsigned char *v = (volatile unsigned char *)p; while (n--) *v++ = 0; }

int devtab_status(DevTable *b, int *code, uint64_t *detail) {
    HIPCHK(hipSetDevice(b->device));
    u32 w = ~0u;
    HIPCHK(hipMemcpy(&w, b->status, sizeof w, hipMemcpyDeviceToHost));
    *code = w == ~0u ? AESGCM_OK : AESGCM_EARG;
    if (detail) *detail = w == ~0u ? 0 : w;
    if (w != ~0u) HIPCHK(hipMemset(b->status, 0xFF, sizeof(u32)));
    return AESGCM_OK;
}

int devtab_destroy(DevTable *b, void *state, size_t wipe_bytes, const char *who) {
    int rc = AESGCM_OK;
    hipError_t e = hipSetDevice(b->device);
    if (e == hipSuccess) e = hipDeviceSynchronize();                       // calls in flight may still use the state
    if (wipe_bytes) {
        if (e == hipSuccess) e = hipMemset(state, 0, wipe_bytes);
        if (e == hipSuccess && b->stage) e = hipMemset(b->stage, 0, b->stage_cap);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (e != hipSuccess) rc = hip_fail(e, who);
    (void)hipFree(state);
    (void)hipFree(b->status);
    if (b->stage) (void)hipFree(b->stage);
    if (b->stage_done) (void)hipEventDestroy(b->stage_done);
    return rc;
}


// Key material of a context from a key (or a pre-expanded schedule): aes_kexp, H, the H-power tables -- k_setup and k_setup_ptab on the context's stream, waited
// for.  The staging buffer for the key bytes belongs to the context (aesgcm_ctx_rekey comes through here without an allocation) and is wiped behind the kernels.
int ctx_load_key(aesgcm_ctx *c, const uint8_t *key, size_t key_len, int pre_nr) {
    hipError_t e;
    if (!c->d_keystage && (e = hipMalloc((void **)&c->d_keystage, 256)) != hipSuccess) return hip_fail(e, "hipMalloc");
    const size_t kb = pre_nr ? (size_t)16 * (pre_nr + 1) : key_len;
    e = hipMemcpyAsync(c->d_keystage, key, kb, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        e = klaunch_setup(c->stream, c->km, c->tables, c->d_keystage, (int)key_len, pre_nr, (u32)c->G);
    }
    if (e == hipSuccess) e = hipMemsetAsync(c->d_keystage, 0, 256, c->stream);    // do not leave key bytes behind
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(e, "k_setup");
    c->nr = pre_nr ? pre_nr : (int)(key_len / 4 + 6);                               // only now: a load that failed leaves the context's round count with its old key material
    return AESGCM_OK;
}

int ctx_create_common(aesgcm_ctx **out, int device, const uint8_t *key, size_t key_len, int pre_nr) {
    if (!out || !key) return AESGCM_EARG;
    *out = nullptr;
    DeviceState *ds;
    int rc = device_state(device, &ds);
    if (rc) return rc;
    rc = set_lds_attrs(device, ds);
    if (rc) return rc;
    aesgcm_ctx *c = new (std::nothrow) aesgcm_ctx();
    if (!c) return AESGCM_ENOMEM;
    c->device = device;
    c->tables = ds->tables;
    c->nr = pre_nr ? pre_nr : (int)(key_len / 4 + 6);
    const int per_cu = 2;
    int G = per_cu * ds->n_cu;
    if (G > AESGCM_GMAX) G = AESGCM_GMAX;
    if (G < 1) G = 1;
    c->G = G;
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) { delete c; return hip_fail(e, "hipSetDevice"); }
    {   // a stream a destroyed context left behind, or a new one
        std::lock_guard<std::mutex> lk(g_mu);
        if (!ds->streams.empty()) { c->stream = ds->streams.back(); ds->streams.pop_back(); }
    }
    if (!c->stream && (e = hipStreamCreate(&c->stream)) != hipSuccess) { delete c; return hip_fail(e, "hipStreamCreate"); }
    if ((e = hipMalloc(&c->km, sizeof(KeyMaterial))) != hipSuccess ||
        (e = hipMalloc(&c->fold_a, sizeof(uint4) * 64 * FOLD_A_ITEMS)) != hipSuccess ||
        (e = hipMalloc(&c->fold_b, sizeof(uint4) * 64 * FOLD_B_ITEMS)) != hipSuccess ||
        (e = hipMalloc(&c->d_counter, 64 * (1 + 2 * AESGCM_NQ))) != hipSuccess ||
        (e = hipMemset(c->d_counter, 0, 64 * (1 + 2 * AESGCM_NQ))) != hipSuccess ||
        (e = hipMalloc(&c->d_cyc, 8 * (2 * CYC_ACC_SLOTS + 1))) != hipSuccess ||
        (e = hipMemset(c->d_cyc, 0, 8 * (2 * CYC_ACC_SLOTS + 1))) != hipSuccess ||
        (e = hipMalloc(&c->d_tag, sizeof(uint4) * 4)) != hipSuccess ||
        (e = hipHostMalloc((void **)&c->h_tag, 64, hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess ||
        (e = hipHostGetDevicePointer((void **)&c->h_tag_dev, c->h_tag, 0)) != hipSuccess ||
        (memset(c->h_tag, 0, 64), false) ||
        (e = hipMalloc(&c->d_trace, sizeof(u64) * 4 * AESGCM_GMAX)) != hipSuccess) { ctx_destroy(c); return hip_fail(e, "hipMalloc"); }
    if ((rc = ctx_load_key(c, key, key_len, pre_nr))) { ctx_destroy(c); return rc; }
    { std::lock_guard<std::mutex> lk(g_mu); g_ctxs.push_back(c); }
    *out = c;
    return AESGCM_OK;
}

// ... and everything a context owns given back (also a half-built one: ctx_create_common's failures come through here); its stream stays with the device
int ctx_destroy(aesgcm_ctx *c) {
    if (!c) return AESGCM_OK;
    { std::lock_guard<std::mutex> lk(g_mu); g_ctxs.erase(std::remove(g_ctxs.begin(), g_ctxs.end(), c), g_ctxs.end()); }
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->ev_session) { hipEventSynchronize(c->ev_session); hipEventDestroy(c->ev_session); }      // (a session's last chunk may be on a caller's stream)
    for (auto &e : c->ev) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    for (auto &e : c->ev_pool) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    if (c->km) { hipMemset(c->km, 0, sizeof(KeyMaterial)); hipFree(c->km); }
    if (c->d_keystage) hipFree(c->d_keystage);
    if (c->parts) hipFree(c->parts);
    if (c->fold_a) hipFree(c->fold_a);
    if (c->fold_b) hipFree(c->fold_b);
    if (c->d_counter) hipFree(c->d_counter);
    if (c->d_cyc) hipFree(c->d_cyc);
    if (c->d_tag) hipFree(c->d_tag);
    if (c->h_tag) hipHostFree(c->h_tag);
    if (c->h_mtag) hipHostFree(c->h_mtag);
    if (c->d_mtag) hipFree(c->d_mtag);
    if (c->d_trace) hipFree(c->d_trace);
    if (c->rows_buf) hipFree(c->rows_buf);
    if (c->side) { hipStreamSynchronize(c->side); hipStreamDestroy(c->side); }
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    if (c->ev_join) hipEventDestroy(c->ev_join);
    pipeline_release(c);
    if (c->st_in) hipFree(c->st_in);
    if (c->st_out) hipFree(c->st_out);
    if (c->st_aad) hipFree(c->st_aad);
    if (c->ev_sync) hipEventDestroy(c->ev_sync);
    if (c->ev_fused) hipEventDestroy(c->ev_fused);
    if (c->stream) {                                            // idle by now (synchronised above): kept for the device's next context, up to 64 of them
        std::lock_guard<std::mutex> lk(g_mu);
        if (c->device >= 0 && c->device < (int)g_dev.size() && g_dev[c->device].streams.size() < 64) { g_dev[c->device].streams.push_back(c->stream); c->stream = nullptr; }
    }
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return AESGCM_OK;
}


// ---------------------------------------------------------------- host-pointer wrappers
int stage_in(aesgcm_ctx *c, const uint8_t *aad, size_t aad_len, const uint8_t *in, size_t len) {
    int rc;
    if ((rc = grow(&c->st_aad, &c->st_aad_cap, aad_len))) return rc;
    if ((rc = grow(&c->st_in, &c->st_in_cap, len))) return rc;
    if ((rc = grow(&c->st_out, &c->st_out_cap, len))) return rc;
    if (aad_len) HIPCHK(hipMemcpyAsync(c->st_aad, aad, aad_len, hipMemcpyHostToDevice, c->stream));
    if (len) HIPCHK(hipMemcpyAsync(c->st_in, in, len, hipMemcpyHostToDevice, c->stream));
    return AESGCM_OK;
}

// A message under way: Y <- 0 and the bookkeeping of aesgcm_ctx::StreamState (aesgcm_stream_begin, the pipelined path, aesgcm_stream_import build on this)
int stream_open(aesgcm_ctx *c, const uint8_t iv[12], int decrypt, hipStream_t st) {
    c->s = aesgcm_ctx::StreamState();
    memcpy(c->s.iv, iv, 12);
    c->s.active = true; c->s.dec = decrypt ? 1 : 0;
    HIPCHK(hipMemsetAsync(c->d_tag + 1, 0, 16, st));
    return AESGCM_OK;
}
// Y' = Y * H^nb ^ P(aad, data) on `st` (NULL: the context's stream).  large: the range may be of any size on device pointers (aesgcm_stream_update_dev) -- it takes the
// launch structure a shard of that size takes (cyclic rows, dealt chunks: MSG_CARRY, aesgcm_msgplan.h); else one k_main launch (chunks that came through the staging buffers).
int stream_absorb(aesgcm_ctx *c, const void *d_aad, u64 aad_len, const void *d_in, u64 len, void *d_out, u64 first_block, hipStream_t st, bool large) {
    const int rc = msg_run(c, MsgCall{MSG_CARRY, c->s.dec ? MODE_DEC : MODE_ENC, c->s.iv, d_aad, aad_len, d_in, len, d_out, first_block, c->d_tag + 1, 0, !large}, st ? st : c->stream);
    if (!rc) c->s.blocks += (aad_len + 15) / 16 + (len + 15) / 16;
    return rc;
}


// ---------------------------------------------------------------- shapes of the packet kernels
#ifdef AESGCM_DEBUG_KNOBS
// Test / profiling builds only (libaesgcm_hip_dbg.so, -DAESGCM_DEBUG_KNOBS; include/aesgcm_debug.h): force the kernel shape the next launches take, so that every
// shape can be checked on inputs the host's own rule would give to another.  The product library has no such switch and reads no environment.
ForceShape g_force = {0, 0, 0, 0, 0, 0, 0};
extern "C" __attribute__((visibility("default"))) int aesgcm_debug_force_shape(const char *what, int value) {
    if (!what) return AESGCM_EARG;
    if (!strcmp(what, "pkt_lanes")) { if (value != 0 && value != 1 && value != 4 && value != 8 && value != 16 && value != 64) return AESGCM_EARG; g_force.pkt_lanes = value; }
    else if (!strcmp(what, "pkt_deal")) g_force.pkt_deal = value;
    else if (!strcmp(what, "batch_lanes")) { if (value != 0 && value != 8 && value != 16 && value != 64) return AESGCM_EARG; g_force.batch_lanes = value; }
    else if (!strcmp(what, "batch_deal")) g_force.batch_deal = value;
    else if (!strcmp(what, "pkt_ilp")) { if (value < 0 || value > 2) return AESGCM_EARG; g_force.pkt_ilp = value; }              // k_pktl's ILP form: 0 = the library's rule, 1 = always, 2 = never
    else if (!strcmp(what, "pkt_rows")) { if (value < 0 || value > 2) return AESGCM_EARG; g_force.pkt_rows = value; }            // aesgcm_packets_crypt_dev by rows (k_rows): 0 = the library's rule, 1 = always, 2 = never
    else if (!strcmp(what, "batch_order")) { if (value < 0 || value > 2) return AESGCM_EARG; g_force.batch_order = value; }      // variable-length batches by length class: 0 = the library's rule, 1 = always, 2 = never
    else return AESGCM_EARG;
    return AESGCM_OK;
}
#endif

// (the shape rules themselves -- packets_pick_lg, batch_pick_lg, the ILP form, the deals, the grid -- are arithmetic: aesgcm_plan.h)
#ifdef AESGCM_DEBUG_KNOBS
// the forced lanes per packet as the kernels' log2, or -1: nothing forced
static int forced_pkt_lg() { const int f = g_force.pkt_lanes; return !f ? -1 : f == 1 ? 0 : f == 64 ? 6 : f == 16 ? 4 : f == 8 ? 3 : 2; }
static int forced_batch_lg() { const int f = g_force.batch_lanes; return !f ? -1 : f == 8 ? 3 : f == 16 ? 4 : 6; }
#endif
// The shape a call takes, as the planners choose it and as the shape queries report it (aesgcm_packets_shape, aesgcm_batch_shape): the rule, or the forced shape
int packets_lg(const aesgcm_ctx *c, size_t n_pkts, size_t pkt_len) {
#ifdef AESGCM_DEBUG_KNOBS
    if (forced_pkt_lg() >= 0) return forced_pkt_lg();
#endif
    return packets_pick_lg((u32)c->G / 2, n_pkts, pkt_len);                  // c->G = two workgroups per CU
}
int batch_lg(const DeviceState *ds, size_t n_pkts, size_t pkt_len, bool var) {
#ifdef AESGCM_DEBUG_KNOBS
    if (forced_batch_lg() >= 0) return forced_batch_lg();
#endif
    return batch_pick_lg(ds->n_cu, n_pkts, pkt_len, var);
}


// The order in which a launch takes packets of mixed length: counting sort by falling length class on the launch's stream (k_len_hist, k_len_scan,
// k_len_scatter).  *perm = NULL when it does not pay or is switched off.  Three launches of about 10 us in front of the packet kernel: mixed frames of
// 64 .. 1514 bytes, AES-256, best shape each (profiles/r04/packets_sweep_mixed_*.txt): 16384 frames 101 GiB/s in array order, 79 by class; 65536 223 / 199; 98304
// 256 / 271; 131072 284 / 320; 262144 382 / 429; 2^20 426 / 717 -- the order pays once the machine is full, and the default threshold is there.
int order_launch(OrderSlot &o, const u64 *d_off, size_t n_pkts, hipStream_t st, const u32 **perm) {
    if (!o.done) HIPCHK(hipEventCreateWithFlags(&o.done, hipEventDisableTiming));
    else HIPCHK(hipStreamWaitEvent(st, o.done, 0));                                // the slot's previous reader, on whatever stream it ran
    // no memory for the scratch (4 bytes per packet): the launch takes the packets as they come -- slower, never wrong
    if (!o.bins && hipMalloc((void **)&o.bins, LEN_SORT_ENTRIES * sizeof(u32)) != hipSuccess) { o.bins = nullptr; (void)hipGetLastError(); *perm = nullptr; return AESGCM_OK; }
    if (o.cap < n_pkts) {
        if (o.perm) { HIPCHK(hipFree(o.perm)); o.perm = nullptr; o.cap = 0; }     // hipFree waits for the launches that may still read it
        if (hipMalloc((void **)&o.perm, n_pkts * sizeof(u32)) != hipSuccess) { o.perm = nullptr; (void)hipGetLastError(); *perm = nullptr; return AESGCM_OK; }
        o.cap = n_pkts;
    }
    LenSrc src = {d_off, nullptr, nullptr, nullptr, 0u};                            // by data length (a batch packet's AAD is short)
    RouteCfg none = {nullptr, (u32)n_pkts, 0u, 0u, 0u, 0u, 0xFFu, 0u, 0, 0, 0, 0, 0, 0};    // a plain order: nothing is routed
    HIPCHK(klaunch_len_sort(st, src, (u32)n_pkts, o.bins, o.perm, none));
    *perm = o.perm;
    return AESGCM_OK;
}


// ---------------------------------------------------------------- many messages under the context's key: by rows (aesgcm_rows.h)
// the scratch of the path, carved out of one allocation: per message 16 + 4 bytes and (offset arrays) the three prefix sums, 32 bytes per record slot.  Zero at rest.
struct RowsScratch { RowsHdr *hdr; u32 *queues; u64 *prefix, *sprefix, *plan_part; u32 *slot_base; RowsRec *rec; unsigned long long *acc; u32 *cnt; u32 *perm, *bins; u64 *bad_part; PktDesc *desc; };

#define ROWS_DESC_MAX_N ((size_t)1 << 24)
size_t rows_carve(unsigned char *base, size_t slots, size_t n, RowsScratch *r) {
    size_t o = 0;
    auto take = [&](size_t bytes) { unsigned char *q = base ? base + o : nullptr; o += (bytes + 255) & ~(size_t)255; return q; };
    RowsScratch t;
    t.hdr = (RowsHdr *)take(sizeof(RowsHdr));
    t.queues = (u32 *)take(64 * ROWS_NQ);
    t.prefix = (u64 *)take(8 * (n + 1));
    t.sprefix = (u64 *)take(8 * (n + 1));
    t.plan_part = (u64 *)take(8 * 4 * (n / 1024 + 2));                   // the planner's sums per workgroup of 1024 messages (units, smalls, slots, first refused length)
    t.slot_base = (u32 *)take(4 * (n + 1));
    t.rec = (RowsRec *)take(sizeof(RowsRec) * slots);
    t.acc = (unsigned long long *)take(16 * n);
    t.cnt = (u32 *)take(4 * n);
    t.perm = (u32 *)take(4 * n);                                         // a routed call: the launch order of the messages that take the packet kernels (k_len_*)
    t.bins = (u32 *)take(4 * (size_t)LEN_SORT_ENTRIES);
    t.bad_part = (u64 *)take(8 * (size_t)LEN_SORT_WGS);                  // ... and the first length each slice of the sort found it cannot take
    t.desc = n <= ROWS_DESC_MAX_N ? (PktDesc *)take(sizeof(PktDesc) * n) : nullptr;      // ... and, for a lane per packet, the launch's packet records (48 bytes each: not for calls of more than 2^24 messages)
    if (r) *r = t;
    return o;
}

int rows_scratch(aesgcm_ctx *c, size_t slots, size_t n, hipStream_t st, RowsScratch *r) {
    if (slots > c->rows_cap_slots || n > c->rows_cap_n) {
        if (c->rows_buf) { HIPCHK(hipFree(c->rows_buf)); c->rows_buf = nullptr; c->rows_cap_slots = c->rows_cap_n = 0; }    // hipFree waits for the launches that may still use it
        const size_t cs = slots < 65536 ? 65536 : slots, cn = n < 4096 ? 4096 : n;
        const hipError_t e = hipMalloc((void **)&c->rows_buf, rows_carve(nullptr, cs, cn, nullptr));
        if (e == hipErrorOutOfMemory) return AESGCM_ENOMEM;
        if (e != hipSuccess) return hip_fail(e, "hipMalloc");
        c->rows_cap_slots = cs; c->rows_cap_n = cn; c->rows_dirty = true;
    }
    if (c->rows_dirty) HIPCHK(hipMemsetAsync(c->rows_buf, 0, rows_carve(nullptr, c->rows_cap_slots, c->rows_cap_n, nullptr), st));   // fresh scratch, or a launch failed half way through a call
    rows_carve(c->rows_buf, c->rows_cap_slots, c->rows_cap_n, r);
    return AESGCM_OK;
}

// The marks of a ROUTED call as length classes (64 bytes each) for k_len_scan: the context's "rows_min" (8 KiB) and a quarter of it -- the two marks packets_by_rows applies
// to fixed-size records, chosen between per call on the device by what lies between them (k_len_scan).  The classes resolve up to 16320 bytes.
static void route_marks(const aesgcm_ctx *c, u32 *c_hi, u32 *c_lo) {
    const u64 hi = c->rows_min / 64, lo = c->rows_min / 4 / 64;
    *c_hi = c->rows_min ? (u32)(hi < PKT_LEN_CLASSES ? hi : PKT_LEN_CLASSES - 1u) : PKT_LEN_CLASSES;      // rows_min = 0: never by rows
    *c_lo = c->rows_min ? (u32)(lo < PKT_LEN_CLASSES ? lo : PKT_LEN_CLASSES - 1u) : PKT_LEN_CLASSES;
#ifdef AESGCM_DEBUG_KNOBS
    if (g_force.pkt_rows == 1) *c_hi = *c_lo = 0;                                          // everything by rows
    else if (g_force.pkt_rows == 2 || g_force.pkt_lanes) *c_hi = *c_lo = PKT_LEN_CLASSES;  // everything through the packet kernels (a forced shape of theirs means them)
#endif
}

// p: the caller's pointers, counts and lengths; the cut and the scratch are filled in here.  k != NULL: the call is ROUTED per message (round 6; the lengths are on the
// device): *k describes the same call for the packet kernels, which take the messages below the mark k_len_scan chooses; the row launches see those as nothing.
int packets_rows(aesgcm_ctx *c, int decrypt, RowsParams &p, hipStream_t st, PktParams *k) {
    const size_t n = p.n_pkts;
    RowsScratch r;
    int rc;
    const bool var = p.data_off != nullptr || p.aad_off != nullptr || p.len_arr != nullptr;          // a length of any kind on the device: the plan is made there
    if (k && !var) return AESGCM_EARG;
    u32 wgs = (u32)c->G / 2;                                                 // one 141 KiB workgroup per CU
    const u32 n_cu = wgs;
    hipStream_t rows_st = st;                                                // where the row launches go: the caller's stream, or (a routed call) the side stream
    size_t slots;
    if (!var) {
        const RowsGeom g = rows_geom(p.pkt_len);
        const u32 na = rows_na(p.aad_len);
        p.U = rows_units(g, na); p.S = rows_smalls(g, na);
        p.G = (u64)n * p.U;
        const u64 need = (p.G + AESGCM_BODY_WG / 64 - 1) / (AESGCM_BODY_WG / 64);     // at least a unit per wave
        if (need < wgs) wgs = (u32)need;
        p.waves = wgs * (AESGCM_BODY_WG / 64);
        rows_cut(p.G, p.waves, c->rows_block, (u64)1 << 30, &p.D, &p.NB, &p.dyn);
        p.SM = p.U ? rows_nat_count(g, na) + (p.U - 1u) / p.D + 1u : 0u;
        if ((u64)n * p.SM >= (1ull << 31)) return AESGCM_ETOOLONG;
        slots = n * p.SM;
    } else {
        p.waves = wgs * (AESGCM_BODY_WG / 64);
        slots = ROWS_SLOTS_PER_MSG * n + ROWS_NB_CAP;                        // a run and a long AAD per message, and one more slot per block boundary inside its rows
        if (slots >= (1ull << 31)) return AESGCM_ETOOLONG;
    }
    if ((rc = rows_scratch(c, slots, n, st, &r))) return rc;
    p.slot_cap = (u32)slots;
    p.rec = r.rec; p.acc = r.acc; p.cnt = r.cnt; p.queues = r.queues;
    c->rows_dirty = true;                                                    // until both launches are enqueued
    if (var) {
        p.hdr = r.hdr; p.prefix = r.prefix; p.sprefix = r.sprefix; p.slot_base = r.slot_base;
        if (k) {
            // the route: a counting sort of the messages by falling size class (data + AAD) whose scan also decides -- which messages go by rows, how many are the packet
            // kernels', and in which shape (aesgcm_rows.h RowsHdr)
            LenSrc src = {p.data_off, p.aad_off, p.len_arr, p.alen_arr, p.aad_len};
            RouteCfg cfg = {r.hdr, (u32)n, n_cu, 0u, 0u, c->route_mid_min, 0xFFu, 0u, c->route_blocks_min, (u64)(uintptr_t)p.in_ptr, (u64)(uintptr_t)p.out_ptr, (u64)(uintptr_t)p.aad_ptr, (u64)(uintptr_t)p.len_arr, (u64)(uintptr_t)p.alen_arr};
            k->scattered = p.len_arr ? 1u : 0u;
            cfg.top_min = c->route_top_min;
            route_marks(c, &cfg.c_hi, &cfg.c_lo);
            const bool probe = decrypt == 2;                                 // aesgcm_frames_ceiling_probe_dev: the packet kernels' instruction stream without the data's traffic -- every message theirs, no row launch
            if (probe) { if (p.len_arr) return AESGCM_EARG; cfg.c_hi = cfg.c_lo = PKT_LEN_CLASSES; }
#ifdef AESGCM_DEBUG_KNOBS
            if (forced_pkt_lg() >= 0) cfg.force_lg = forced_pkt_lg() == 6 && p.len_arr ? 4u : (u32)forced_pkt_lg();      // (messages wherever they live have no wave-per-packet instance: 16 lanes)
            if (g_force.pkt_deal >= 1 && g_force.pkt_deal <= (int)PKTG_MAX_DEAL) cfg.force_deal = (u32)g_force.pkt_deal;
#endif
            // (the sort also checks every length: a call with one of 2^28 bytes or more is refused by its scan -- hdr->bad -- and every launch behind returns at once)
            const DescSrc ds = {r.desc, p.ivs, p.in_ptr, p.out_ptr, p.aad_ptr};                 // (r.desc is NULL beyond 2^24 messages: rows_carve)
            HIPCHK(klaunch_len_sort(st, src, (u32)n, r.bins, r.perm, cfg, r.bad_part, reinterpret_cast<u32 *>(c->h_tag_dev + 2), ds));
            k->perm = r.perm; k->route = r.hdr; k->desc = ds.desc; k->counter = &r.hdr->pkt_counter; k->counter_base = 0; k->plain = 0;
            k->n_pkts = (u32)n;
            // Behind the sort the call FORKS: the row launches (plan, k_rows, k_rows_close) go to the context's side stream, the packet kernels stay on the caller's, and
            // the caller's stream waits for the side stream at the end.  The two halves share nothing but the header the scan left (read-only from here on, except the
            // plan's own fields); a call of frames alone no longer waits for seven launches that find nothing to do.  (The two big launches do not share the chip: k_pktl and
            // k_rows each hold a CU with one 141 KiB workgroup, so k_rows runs when the packet launch ends -- profiles/r06/route_band.txt.)
            if (!probe && !c->side) {
                HIPCHK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
                HIPCHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
                HIPCHK(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
            }
            // after the fork a failing launch still joins before the call returns: the caller's stream is then ordered behind whatever reached the side stream
            // (the scratch stays marked dirty: the next call clears it on that stream)
#define FORKCHK(call) do { hipError_t _e = (call); if (_e != hipSuccess) { if (rows_st != st) { hipEventRecord(c->ev_join, rows_st); hipStreamWaitEvent(st, c->ev_join, 0); } \
                                                                      return hip_fail(_e, #call); } } while (0)
            if (!probe) {
                HIPCHK(hipEventRecord(c->ev_fork, st));
                HIPCHK(hipStreamWaitEvent(c->side, c->ev_fork, 0));
                rows_st = c->side;
                FORKCHK(klaunch_rows_plan(rows_st, p, true, c->rows_block, (u32)ROWS_NB_CAP, r.plan_part, reinterpret_cast<u32 *>(c->h_tag_dev + 2)));
            }
            // every shape the count of small messages -- anything up to n -- could ask for; all but the one k_len_scan named return before they stage a table
            const u32 lg_min = cfg.force_lg != 0xFFu ? cfg.force_lg : route_pick_lg(n_cu, n), lg_max = cfg.force_lg != 0xFFu ? cfg.force_lg : 4u;
            static const u32 shapes[] = {0u, 2u, 3u, 4u, 6u};
            for (u32 lg : shapes) {
                if (lg < lg_min || lg > lg_max || cfg.c_hi == 0u) continue;                  // (c_hi = 0: everything by rows, forced)
                const u32 w = pkt_grid(n_cu, n, (int)lg, false, 64u >> lg).wgs;                 // (the deal is the scan's: the grid is sized for a wave-iteration per fetch)
                if (lg == 0u) FORKCHK(klaunch_pktl(c->nr, decrypt, false, w, st, c->km, c->tables, *k));
                else FORKCHK(klaunch_pktg(c->nr, decrypt, (int)lg, w, st, c->km, c->tables, *k));
            }
            if (probe) { c->rows_dirty = false; return AESGCM_OK; }           // (nothing of the row path ran: its scratch is at rest)
        } else {
            HIPCHK(klaunch_rows_plan(st, p, false, c->rows_block, (u32)ROWS_NB_CAP, r.plan_part, reinterpret_cast<u32 *>(c->h_tag_dev + 2)));
        }
    }
    p.prio_rows = c->cyc_prio;
    if (wgs) FORKCHK(klaunch_rows(c->nr, decrypt, wgs, rows_st, c->km, c->tables, p));                          // (fixed-size records of no bytes and no AAD have no units: their tags are the closing's alone)
    size_t close_lanes = p.slot_cap > n ? p.slot_cap : n;                                                    // a lane per record slot and per message; the lanes stride, so the grid is capped (and with offset arrays most slots of the worst case are never given out)
    if (close_lanes > (size_t)4096 * ROWS_CLOSE_WG) close_lanes = (size_t)4096 * ROWS_CLOSE_WG;
    FORKCHK(klaunch_rows_close(decrypt, (unsigned)((close_lanes + ROWS_CLOSE_WG - 1) / ROWS_CLOSE_WG), rows_st, c->km, c->tables, p));
    if (rows_st != st) { HIPCHK(hipEventRecord(c->ev_join, rows_st)); HIPCHK(hipStreamWaitEvent(st, c->ev_join, 0)); }      // the join
#undef FORKCHK
    c->rows_dirty = false;
    return AESGCM_OK;
}

// Does a call of FIXED-SIZE records go by rows?  (With offset arrays every message is routed by its own size on the device: k_len_scan applies the same two marks per
// message, aesgcm_rows.h.)  From rows_min bytes per packet (8 KiB), and from a quarter of that while the packets are few: the packet kernels need a packet per lane
// (or per lane group) to fill the chip, the rows of a call fill it whatever the count.  Measured on one box with the smalls in the closing launch, AES-256,
// GiB/s by rows / by the packet kernels (profiles/r05/rows_min_sweep2.txt, rows_min_sweep3.txt): 32 KiB x 131072 885 / 721, + 16 bytes 870 / 666; 16 KiB x 262144
// 845 / 792, + 16 827 / 749, x 16384 634 / 563, x 4096 571 / 400; 8 KiB x 524288 770 / 727, + 16 746 / 695, x 32768 596 / 545, x 4096 464 / 254, x 1024 189 / 129;
// 6 KiB x 699050 709 / 802, x 65536 613 / 613, x 8192 501 / 282; 4 KiB x 2^20 620 / 810, x 131072 557 / 667, x 32768 495 / 485, x 16384 502 / 384, x 4096 339 / 151;
// 2 KiB x 2^20 429 / 804, x 16384 352 / 242, x 4096 206 / 115; 1 KiB x 262144 264 / 616, x 4096 116 / 83.
bool packets_by_rows(const aesgcm_ctx *c, size_t n_pkts, size_t pkt_len) {
#ifdef AESGCM_DEBUG_KNOBS
    if (g_force.pkt_rows) return g_force.pkt_rows == 1;
    if (g_force.pkt_lanes) return false;                                     // a forced shape of the packet kernels means the packet kernels
#endif
    if (!c->rows_min) return false;
    if (n_pkts <= 16384) return 4 * pkt_len >= c->rows_min;
    if (pkt_len < c->rows_min) return false;
    // many packets of 8 .. 16 KiB whose last, partial row has more than a few blocks: what is not a whole row costs a message about a row and a half either way (a
    // pass of a wave in the row launch, or a lane per block of the closing launch), and the lane-per-packet kernel keeps them -- 262 144 x 9000 bytes (8 rows + 51
    // blocks) 613 by rows, 768 there; x 8448 (8 rows + 16 blocks) 696 / 821; from 16 KiB rows win again: 131 072 x 16 656 744 / 682
    // (profiles/r05/rows_ragged_many.txt)
    if (pkt_len < 2 * c->rows_min && rows_geom(pkt_len).tb > ROWS_FEW_TAIL) return false;
    return true;
}

// Fixed-size records through the packet kernels: the shape, its form, the deal and the grid (aesgcm_plan.h), and the context's dispenser -- p.counter_base is where
// the launch finds it, c->counter_base where it leaves it.  p: the caller's pointers, counts and lengths.
void packets_plan(aesgcm_ctx *c, PktParams &p, PacketsPlan &b) {
    const u32 n_cu = (u32)c->G / 2;                                                 // c->G = two workgroups per CU
    const size_t n_pkts = p.n_pkts, pkt_len = p.pkt_len;
    b.lg = packets_lg(c, n_pkts, pkt_len);
    p.counter = c->d_counter; p.counter_base = c->counter_base;
    if (b.lg == 0) {
        b.ilp = pktl_pick_ilp(n_cu, n_pkts, pkt_len);
#ifdef AESGCM_DEBUG_KNOBS
        if (g_force.pkt_ilp) b.ilp = g_force.pkt_ilp == 1;
#endif
    } else {
        p.plain = pktg_is_plain(b.lg, p.aad_off || p.aad_len, p.aligned != 0, pkt_len);
        p.deal = pktg_pick_deal(n_cu, b.lg, n_pkts);
#ifdef AESGCM_DEBUG_KNOBS
        const u32 P = 64u >> b.lg;                                                  // packets per wave-iteration
        if (g_force.pkt_deal >= 1 && g_force.pkt_deal <= (int)PKTG_MAX_DEAL) p.deal = ((u32)g_force.pkt_deal + P - 1) / P * P;
#endif
    }
    const PktGrid g = pkt_grid(n_cu, n_pkts, b.lg, b.ilp, p.deal);
    b.wgs = g.wgs;
    c->counter_base += g.nb + g.wgs * g.waves_per_wg;                               // every wave ends on one failing fetch
}
int packets_launch(aesgcm_ctx *c, int decrypt, PktParams &p, hipStream_t st) {
    PacketsPlan b;
    packets_plan(c, p, b);
    const hipError_t le = b.lg == 0 ? klaunch_pktl(c->nr, decrypt, b.ilp, b.wgs, st, c->km, c->tables, p) : klaunch_pktg(c->nr, decrypt, b.lg, b.wgs, st, c->km, c->tables, p);
    if (le != hipSuccess) { c->counter_base = p.counter_base; return hip_fail(le, "k_pkt launch"); }      // nothing ran: the dispenser stands where it stood
    return AESGCM_OK;
}

thread_local const RowsHdr *g_wipe_hdr = nullptr;
// zero the output of every packet whose d_auth[] entry is 0 (behind the launch that wrote it, on the same stream)
int wipe_failed(int device, size_t n_pkts, void *d_out, size_t pkt_len, const u64 *d_data_off, const int *d_auth, hipStream_t st, const u64 *d_out_ptr, const u32 *d_len, const RowsHdr *hdr) {
    if (!n_pkts || !d_auth || (!d_out && !d_len)) return AESGCM_OK;
    HIPCHK(hipSetDevice(device));
    g_wipe_hdr = hdr;
    const hipError_t e = klaunch_wipe_failed(st, (unsigned char *)d_out, d_auth, d_data_off, (u32)n_pkts, (u32)pkt_len, d_out_ptr, d_len);
    g_wipe_hdr = nullptr;
    HIPCHK(e);
    return AESGCM_OK;
}


// ---------------------------------------------------------------- batch (per-packet key and IV)
// Variable-length batches by length class: mixed frames of 64 .. 1514 bytes, GiB/s in array order / by class (profiles/r04/batch_mixed_*.txt): AES-128 65536 packets
// 202 / 178, 262144 313 / 307, 393216 332 / 342, 2^20 362 / 493; AES-256 65536 177 / 167, 98304 205 / 213, 262144 266 / 290, 2^20 301 / 437.
#define BATCH_ORDER_MIN(nr) ((nr) == 10 ? 262144u : 98304u)
int batch_plan(int device, int decrypt, size_t n_pkts, size_t key_len, BatchParams &p, void *stream, BatchPlan &b) {
    if (key_len != 16 && key_len != 24 && key_len != 32) return AESGCM_EKEYLEN;
    if (n_pkts >= (((size_t)1) << 31)) return AESGCM_ETOOLONG;
    DeviceState *ds;
    int rc = device_state(device, &ds);
    if (rc) return rc;
    if ((rc = set_lds_attrs(device, ds))) return rc;
    HIPCHK(hipSetDevice(device));
    p.n_pkts = (u32)n_pkts;
    {   // a fresh dispenser per launch (zeroed on the launch stream), so launches on different streams may overlap
        std::lock_guard<std::mutex> lk(g_mu);
        p.counter = ds->batch_counter + (ds->batch_slot++ % BATCH_DISPENSERS);
        p.counter_base = 0;
    }
    const int nr = (int)(key_len / 4 + 6);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(p.counter, 0, 4, st));
    const int lg = batch_lg(ds, n_pkts, p.pkt_len, p.data_off != nullptr);                // k_batch3 with 8 / 16 / 64 lanes per packet
    if (decrypt == 2 && lg != 3) { snprintf(g_err, sizeof g_err, "the probe of the batch kernel exists in the 8-lanes-per-packet shape; this call takes %d", 1 << lg); return AESGCM_EARG; }
    // packets of mixed length: by falling length class once the batch fills the machine several times over (BATCH_ORDER_MIN; as aesgcm_packets_crypt_dev)
    bool ordered = lg < 6 && p.data_off && n_pkts >= BATCH_ORDER_MIN(nr);
#ifdef AESGCM_DEBUG_KNOBS
    if (g_force.batch_order) ordered = lg < 6 && p.data_off && g_force.batch_order == 1;
#endif
    if (ordered) {
        // A stream that is being captured takes the packets in array order, as a call without memory for the order does: slower, never wrong.  The order's scratch
        // belongs to the device, not to the graph -- a later, larger call frees it under a graph that would hold its address -- and neither the slot's event nor an
        // allocation belongs into a capture.  Asked only here: a call that would not be ordered pays nothing.  (include/aesgcm.h, CAPTURE)
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing) HIPCHK(hipStreamIsCapturing(st, &cap));         // a weak reference (above): a runtime without stream capture has no stream that captures
        if (cap != hipStreamCaptureStatusNone) ordered = false;
    }
    if (ordered) {
        b.order_lock = std::unique_lock<std::mutex>(g_mu);                        // held from the choice of the slot to the event behind its reader: callers on other threads queue up here
        b.oslot = &ds->order[ds->order_next++ & 3u];
        if ((rc = order_launch(*b.oslot, p.data_off, n_pkts, st, &p.perm))) return rc;
    }
    p.plain = batch_is_plain(lg, p.data_off || p.aad_off || p.aad_len, p.aligned != 0, p.pkt_len);
    const u32 waves_per_wg = (u32)BATCH3_LANES(nr) / 64;
    const u32 P = 64u >> lg, per_wg = waves_per_wg * P;
    u32 wgs = (u32)((n_pkts + per_wg - 1) / per_wg);
    if (wgs > (u32)ds->n_cu) wgs = (u32)ds->n_cu;
    p.deal = batch_pick_deal(wgs, waves_per_wg, lg, n_pkts);
#ifdef AESGCM_DEBUG_KNOBS
    if (g_force.batch_deal >= 1 && g_force.batch_deal <= 4096) p.deal = ((u32)g_force.batch_deal + P - 1) / P * P;
#endif
    b.nr = nr; b.lg = lg; b.wgs = wgs; b.st = st; b.tables = ds->tables;
    return AESGCM_OK;
}
int batch_done(const BatchPlan &b, const BatchParams &p) {
    if (b.oslot && p.perm) HIPCHK(hipEventRecord(b.oslot->done, b.st));
    return AESGCM_OK;
}
int batch_launch(int device, int decrypt, size_t n_pkts, size_t key_len, BatchParams &p, void *stream) {
    BatchPlan b;
    const int rc = batch_plan(device, decrypt, n_pkts, key_len, p, stream, b);
    if (rc) return rc;
    HIPCHK(klaunch_batch3(b.nr, decrypt, b.lg, b.wgs, b.st, b.tables, p));
    return batch_done(b, p);
}


// ---------------------------------------------------------------- pipelined host-buffer path
// H2D of chunk k+1, the fused kernel on chunk k and D2H of chunk k-1 overlap on three streams; the GHASH
// value is carried from chunk to chunk on the device (Y' = Y*H^blocks ^ P, the same combine the beat-by-beat
// interface uses), so the result is bit-identical to one launch over the whole message.
void pipeline_release(aesgcm_ctx *c) {
    for (int i = 0; i < 2; i++) {
        if (c->pl_buf[i]) { hipFree(c->pl_buf[i]); c->pl_buf[i] = nullptr; }
        if (c->pl_ev_h2d[i]) { hipEventDestroy(c->pl_ev_h2d[i]); c->pl_ev_h2d[i] = nullptr; }
        if (c->pl_ev_k[i]) { hipEventDestroy(c->pl_ev_k[i]); c->pl_ev_k[i] = nullptr; }
        if (c->pl_ev_d2h[i]) { hipEventDestroy(c->pl_ev_d2h[i]); c->pl_ev_d2h[i] = nullptr; }
    }
    if (c->pl_in) { hipStreamDestroy(c->pl_in); c->pl_in = nullptr; }
    if (c->pl_out) { hipStreamDestroy(c->pl_out); c->pl_out = nullptr; }
    c->pl_cap = 0;
}

// all or nothing: either both streams, all six events and both chunk slots of `chunk` bytes exist afterwards, or none
// of them does (pl_in == NULL, pl_cap == 0) and the next call starts from scratch
int pipeline_prepare(aesgcm_ctx *c, size_t chunk) {
    hipError_t e = hipSuccess;
    if (!c->pl_in) {
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->pl_in, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->pl_out, hipStreamNonBlocking);
        for (int i = 0; i < 2 && e == hipSuccess; i++) {
            e = hipEventCreateWithFlags(&c->pl_ev_h2d[i], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&c->pl_ev_k[i], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&c->pl_ev_d2h[i], hipEventDisableTiming);
        }
        if (e != hipSuccess) { pipeline_release(c); return hip_fail(e, "pipeline streams/events"); }
    }
    if (chunk > c->pl_cap) {
        c->pl_cap = 0;
        for (int i = 0; i < 2 && e == hipSuccess; i++) {
            if (c->pl_buf[i]) { e = hipFree(c->pl_buf[i]); c->pl_buf[i] = nullptr; }
            if (e == hipSuccess) e = hipMalloc((void **)&c->pl_buf[i], chunk);
        }
        if (e != hipSuccess) {
            pipeline_release(c);
            return e == hipErrorOutOfMemory ? AESGCM_ENOMEM : hip_fail(e, "pipeline chunk slots");
        }
        c->pl_cap = chunk;
    }
    return AESGCM_OK;
}


int crypt_pipelined(aesgcm_ctx *c, int dec, const uint8_t iv[12], const uint8_t *aad, size_t aad_len,
                           const uint8_t *in, size_t len, uint8_t *out, uint8_t tag[16], size_t chunk) {
    int rc = check_lengths(aad_len, len);
    if (rc) return rc;
    // the chunk-to-chunk GHASH value lives in the streaming slot (d_tag[1], s_iv, s_dec): refuse to run inside an open
    // stream_begin .. stream_final session instead of silently corrupting its running GHASH
    if (c->s.active) return AESGCM_ESTATE;
    if (!chunk) chunk = (size_t)64 << 20;
    chunk = (chunk + 1023) / 1024 * 1024;                    // whole rows, 16-byte aligned chunk starts
    if (chunk > len) chunk = (len + 1023) / 1024 * 1024;
    if (!chunk) chunk = 1024;
    HIPCHK(hipSetDevice(c->device));
    if ((rc = pipeline_prepare(c, chunk))) return rc;
    // state Y <- 0, then the AAD (small; through the staging buffer on the compute stream): the same StreamState the beat-by-beat interface keeps, open for the
    // length of this call
    if ((rc = stream_open(c, iv, dec, c->stream))) return rc;
    struct Close { aesgcm_ctx *c; ~Close() { c->s.active = false; } } close_on_return{c};
    if (aad_len) {
        if ((rc = stage_in(c, aad, aad_len, nullptr, 0))) return rc;
        if ((rc = stream_absorb(c, c->st_aad, aad_len, c->st_in, 0, c->st_out, 0))) return rc;
    }
    const size_t n_chunks = (len + chunk - 1) / chunk;
    for (size_t k = 0; k < n_chunks; k++) {
        const int s = (int)(k & 1);
        const size_t off = k * chunk, m = (len - off < chunk) ? len - off : chunk;
        if (k >= 2) HIPCHK(hipStreamWaitEvent(c->pl_in, c->pl_ev_d2h[s], 0));     // slot free again
        HIPCHK(hipMemcpyAsync(c->pl_buf[s], in + off, m, hipMemcpyHostToDevice, c->pl_in));
        HIPCHK(hipEventRecord(c->pl_ev_h2d[s], c->pl_in));
        HIPCHK(hipStreamWaitEvent(c->stream, c->pl_ev_h2d[s], 0));
        if ((rc = stream_absorb(c, nullptr, 0, c->pl_buf[s], m, c->pl_buf[s], off / 16))) return rc;   // in place
        HIPCHK(hipEventRecord(c->pl_ev_k[s], c->stream));
        HIPCHK(hipStreamWaitEvent(c->pl_out, c->pl_ev_k[s], 0));
        HIPCHK(hipMemcpyAsync(out + off, c->pl_buf[s], m, hipMemcpyDeviceToHost, c->pl_out));
        HIPCHK(hipEventRecord(c->pl_ev_d2h[s], c->pl_out));
    }
    if ((rc = launch_combine(c, plan_combine_final(c->d_tag + 1, iv, aad_len, len, c->d_tag), c->stream))) return rc;
    if ((rc = fetch_tag(c, c->stream, tag))) return rc;
    HIPCHK(hipStreamSynchronize(c->pl_out));
    return AESGCM_OK;
}
