// aesgcm_wire_kernels.hip -- key tables on frames in wire format (gfx950): aesgcm_keytab_frames_crypt_dev's kernel and its launcher; the host side is aesgcm_keytab.hip.
//
//   k_kt_wire<NR,DEC,LG>    k_kt_batch's loop (aesgcm_batch3_body.inc, SLOTS = true, WIRE = true) on frames header | payload | ICV packed in one buffer: the lane group
//                           takes AAD range, payload range, nonce and ICV position from the frame's one offset and the call's aesgcm_wire_fmt (a kernel parameter),
//                           builds J0 from the slot's salt and header bytes, and writes or compares the truncated ICV inside the frame -- no IV, offset or tag arrays, and
//                           no second pass over headers and ICVs.  A frame it cannot take -- slot out of range or unset, offsets falling, 2^28 bytes or more, shorter than
//                           header + ICV -- reads nothing but its slot number and offsets: output untouched, auth 0, its index into the table's status word.
// A translation unit of its own: its ISA census (`make asm_wire`) is read apart from the key tables' (`make asm_keytab`).
#include "aesgcm_keytab.h"
#include "aesgcm_lanes.h"
#include "aesgcm_wirecut.h"
#include "aesgcm_dispatch.h"

template <int NR, int DEC, int LG>                       // DEC: 0 encrypt, 1 decrypt
__global__ __launch_bounds__(BATCH3_LANES(NR), (BATCH3_LANES(NR) + 255) / 256) void k_kt_wire(const DevTables *__restrict__ tb, const KtWireParams wp) {
    constexpr bool SLOTS = true, WIRE = true;            // key material from the slots of kt, packets laid out by wf
    const KtParams *const kt = &wp.k;
    const BatchParams &p = wp.k.b;
    const aesgcm_wire_fmt *const wf = &wp.f;
    constexpr u32 WIREX = 0;                            // every nonce and AAD byte is a frame byte or the slot's salt (otherwise: aesgcm_wirex_kernels.hip)
    constexpr const KtWireXParams *wx = nullptr;
#include "aesgcm_batch3_body.inc"
}

// ------------------------------------------------------------------------------------------------ launchers
hipError_t klaunch_wire_attributes() {
    return batch3_each([](auto NR, auto D, auto LG) { return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_wire<NR(), D(), LG()>), hipFuncAttributeMaxDynamicSharedMemorySize, BATCH3_LDS_BYTES_LG(LG())); });
}

hipError_t klaunch_kt_wire(int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtWireParams &p) {
    batch3_dispatch(nr, dec, lg, [&](auto NR, auto D, auto LG) { hipLaunchKernelGGL((k_kt_wire<NR(), D(), LG()>), dim3(wgs), dim3(BATCH3_LANES(NR())), BATCH3_LDS_BYTES_LG(LG()), st, tb, p); });
    return hipGetLastError();
}
