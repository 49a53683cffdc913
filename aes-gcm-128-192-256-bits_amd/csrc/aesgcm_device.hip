// aesgcm_device.hip -- the library's ONE device translation unit: libaesgcm_hip.so carries a single gfx950 code object (tests/test_abi_cpu.py lists the offload
// bundle's entries), so every kernel source is compiled here together.  Each source still compiles on its own for its ISA census
// (`make asm` for aesgcm_kernels.hip, `make asm_<family>` for aesgcm_<family>_kernels.hip).
#include "aesgcm_kernels.hip"
#include "aesgcm_keytab_kernels.hip"
#include "aesgcm_wire_kernels.hip"
#include "aesgcm_wirex_kernels.hip"
#include "aesgcm_tls_kernels.hip"
#include "aesgcm_quic_kernels.hip"
#include "aesgcm_dtls_kernels.hip"
#include "aesgcm_srtp_kernels.hip"
#include "aesgcm_rxwin_kernels.hip"
#include "aesgcm_txnum_kernels.hip"
#include "aesgcm_kdf_kernels.hip"
#include "aesgcm_srtp_kdf_kernels.hip"
#include "aesgcm_prf12_kernels.hip"
#include "aesgcm_prfplus_kernels.hip"
#include "aesgcm_mka_kernels.hip"
