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
#define ATTRCHK(call) do { const hipError_t _e = (call); if (_e != hipSuccess) return _e; } while (0)
#define SETATTRW(NR, D) ATTRCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_wire<NR, D, 6>), hipFuncAttributeMaxDynamicSharedMemorySize, BATCH3_LDS_BYTES_LG(6))); \
                        ATTRCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_wire<NR, D, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, BATCH3_LDS_BYTES_LG(4))); \
                        ATTRCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_wire<NR, D, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, BATCH3_LDS_BYTES_LG(3)))
    SETATTRW(10, 0); SETATTRW(12, 0); SETATTRW(14, 0); SETATTRW(10, 1); SETATTRW(12, 1); SETATTRW(14, 1);
#undef SETATTRW
#undef ATTRCHK
    return hipSuccess;
}

hipError_t klaunch_kt_wire(int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtWireParams &p) {
#define LKW(NR, D, LG) hipLaunchKernelGGL((k_kt_wire<NR, D, LG>), dim3(wgs), dim3(BATCH3_LANES(NR)), BATCH3_LDS_BYTES_LG(LG), st, tb, p)
#define LKWN(D, LG) do { if (nr == 10) LKW(10, D, LG); else if (nr == 12) LKW(12, D, LG); else LKW(14, D, LG); } while (0)
    if (lg == 3) { if (dec) LKWN(1, 3); else LKWN(0, 3); }
    else if (lg == 4) { if (dec) LKWN(1, 4); else LKWN(0, 4); }
    else { if (dec) LKWN(1, 6); else LKWN(0, 6); }
#undef LKWN
#undef LKW
    return hipGetLastError();
}
