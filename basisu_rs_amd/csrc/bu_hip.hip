// gfx950 kernels and the C ABI (include/basisu_hip.h) of the UASTC / ETC1S block-transcode path.
//
// Data layout in HBM
//   UASTC slice      n x 16-byte blocks, raster order (uastc.rs:49-75)            -> read once as uint4
//   ASTC/BC7/ETC2    n x 16-byte blocks, same order                                -> written once as uint4
//   ETC1             n x  8-byte blocks                                            -> uint2
//   RGBA32           row-major image, pitch 16*blocks_per_row bytes (uastc.rs:96) -> 4 x uint4 per block
//   tables           one BuTables blob (9.5 KiB); every workgroup copies the ranges its target reads to LDS
// Mapping: one lane = one block.  A wave reads 64 x 16 B = 1 KiB contiguous and writes 1 KiB (512 B
// for ETC1; for RGBA32 four 1 KiB row segments when the row has >= 64 blocks).  No MFMA: the work is
// bit-field surgery on 128-bit values.  The roofline is HBM (bytes per block); what limits the kernels
// in practice is vector-ALU instruction issue.
//
// One translation unit; the pieces, in inclusion order, are listed at the bottom of this file.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <future>
#include <iterator>
#include <mutex>
#include <new>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/basisu_hip.h"
#include "bu_basis.hpp"
#include "bu_batch_plan.hpp"   // slices -> runs -> launches of the batch entry points (host only)
#include "bu_uastc_dispatch.hpp"
#include "bu_etc1s_targets.hpp"   // ETC1S per block: index check, ETC1, RGBA32, BC1 / BC3 / BC4 / BC5 / EAC R11 / RG11 (palette form)
#include "bu_decode_blocks.hpp"   // block decoders: the ten block formats -> 16 RGBA8 texels
#include "bu_encode_blocks.hpp"   // block encoders from pixels: 16 RGBA8 texels -> BC4 / BC5 / EAC R11 / RG11 / BC1 / BC3, and the gather of a block's texels
#include "bu_uastc_encode.hpp"    // the UASTC encoder from pixels: 16 RGBA8 texels -> one UASTC block
#include "bu_launch_plan.hpp"  // kernel, grid and arguments of every UASTC launch (host only)
#include "bu_rect_plan.hpp"    // rectangles of slices into pitched surfaces: job table, address mapping, launch plan
#include "bu_etc1s_rect_plan.hpp"  // the same for ETC1S slices: 64-block units, a wave each
#include "bu_multi_addr.hpp"   // the multi-run launch: run cursor, tile corner, lane offsets (one copy for the kernel and the host tests)
#include "bu_file_layout.hpp"  // whole files: ETC1S index buffer and slice table, UASTC runs and pieces, the CRC fold (host only)
#include "bu_etc1s_stream.hpp" // whole ETC1S files, streamed: the scheduler of decoders and feeder behind a device sink (host only)

#include "bu_kernels.hpp"        // device code: UASTC, status reset, CRC, sleep, copy
#include "bu_etc1s_kernels.hpp"  // device code: the ETC1S back end
#include "bu_decode_kernels.hpp" // device code: blocks -> RGBA8 image
#include "bu_encode_kernels.hpp" // device code: RGBA8 image -> blocks
#include "bu_uastc_encode_kernels.hpp" // device code: RGBA8 image -> UASTC blocks
#include "bu_context.hpp"        // bu_context, error / drain / reservation helpers (HIP runtime API only, no kernel)
#include "bu_staged_call.hpp"    // the protocol of the blocking host-pointer entry points (HIP runtime API only, no kernel)
#include "bu_uastc_launch.hpp"   // kernel tables, launcher of one UASTC slice, host-pointer UASTC driver
#include "bu_streams.hpp"        // the context's own streams (hardware-queue check), BU_LAUNCH_AUTO
#include "bu_capi_slice.hpp"     // extern "C": slice level
#include "bu_capi_file.hpp"      // extern "C": whole-file level
#include "bu_capi_measure.hpp"   // extern "C": measurement helpers
#include "bu_multi.hpp"          // extern "C": multi-GPU
#include "bu_capi_decode.hpp"    // extern "C": blocks of the ten block formats -> RGBA8
#include "bu_capi_encode.hpp"    // extern "C": an RGBA8 image -> blocks of the six formats with an encoder from texels, and -> UASTC blocks
