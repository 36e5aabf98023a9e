// Per-block entry point of the UASTC kernels: 7-bit mode code -> mode-specialised transcoder.
// Targets mirror uastc::TargetTextureFormat (uastc.rs:41-47) plus the RGBA32 unpack (uastc.rs:89-110).
#pragma once
#include "bu_uastc_astc.hpp"
#include "bu_uastc_bc7.hpp"
#include "bu_uastc_etc.hpp"
#include "bu_uastc_channel.hpp"
#include "bu_uastc_colour.hpp"

enum { BU_TGT_ASTC = 0, BU_TGT_BC7 = 1, BU_TGT_ETC1 = 2, BU_TGT_ETC2 = 3, BU_TGT_RGBA = 4,
       BU_TGT_BC4 = 6, BU_TGT_BC5 = 7, BU_TGT_R11 = 8, BU_TGT_RG11 = 9,  // (6..9: one- and two-channel targets, bu_uastc_channel.hpp; 5 names none)
       BU_TGT_BC1 = 11, BU_TGT_BC3 = 12 };  // (11, 12: colour targets, bu_uastc_colour.hpp; 10 names none)
constexpr bool bu_channel_target(int target) { return target >= BU_TGT_BC4 && target <= BU_TGT_RG11; }
constexpr bool bu_colour_target(int target) { return target == BU_TGT_BC1 || target == BU_TGT_BC3; }
// the targets encoded per block after the RGBA32 unpack: the one- and two-channel targets and the colour targets
constexpr bool bu_after_rgba(int target) { return bu_channel_target(target) || bu_colour_target(target); }
// result words per block: 16 (RGBA32), 2 (the 8-byte targets ETC1, BC4, EAC R11, BC1) or 4
constexpr int bu_out_words(int target)
{
    return target == BU_TGT_RGBA ? 16 : (target == BU_TGT_ETC1 || target == BU_TGT_BC4 || target == BU_TGT_R11 || target == BU_TGT_BC1) ? 2 : 4;
}
// The targets encoded after the RGBA32 unpack are launched as the ETC family is (bu_launch_plan.hpp): vector-ALU bound, no tile tickets; the
// 8-byte ones in ETC1's shapes, the 16-byte ones in ETC2's.  Every other target is its own.
constexpr int bu_shape_target(int target) { return !bu_after_rgba(target) ? target : bu_out_words(target) == 2 ? BU_TGT_ETC1 : BU_TGT_ETC2; }
constexpr bool bu_etc_family(int target) { return bu_shape_target(target) == BU_TGT_ETC1 || bu_shape_target(target) == BU_TGT_ETC2; }
// the row of BU_COST_ORDER / key_lut a target's mode-sorted kernel sorts by: the targets encoded after the RGBA32 unpack sort as RGBA32
constexpr int bu_cost_row(int target) { return bu_after_rgba(target) ? BU_TGT_RGBA : target; }

template <int TARGET, int M>
BU_DEV int bu_block_mode(const BuTables& T, const BuBlk& b, uint32_t* out)
{
    if constexpr (TARGET == BU_TGT_ASTC) return bu_block_astc<M>(T, b, out);
    else if constexpr (TARGET == BU_TGT_BC7) return bu_block_bc7<M>(T, b, out);
    else if constexpr (TARGET == BU_TGT_ETC1) return bu_block_etc<M, false>(T, b, out);
    else if constexpr (TARGET == BU_TGT_ETC2) return bu_block_etc<M, true>(T, b, out);
    else if constexpr (TARGET == BU_TGT_RGBA) return bu_block_rgba<M>(T, b, out);
    else if constexpr (bu_channel_target(TARGET))
        return bu_block_channels<M, TARGET == BU_TGT_BC4 || TARGET == BU_TGT_BC5, TARGET == BU_TGT_BC5 || TARGET == BU_TGT_RG11>(T, b, out);
    else return bu_block_colour<M, TARGET == BU_TGT_BC3>(T, b, out);
}

// out: bu_out_words(TARGET) words: 4 (ASTC/BC7/ETC2/BC5/RG11/BC3), 2 (ETC1/BC4/R11/BC1) or 16 (RGBA, row-major texels of the block)
template <int TARGET>
BU_DEV int bu_block_any(const BuTables& T, uint32_t mode, const BuBlk& b, uint32_t* out)
{
    switch (mode) {
#define BU_CASE(m) \
    case m: return bu_block_mode<TARGET, m>(T, b, out);
        BU_CASE(0) BU_CASE(1) BU_CASE(2) BU_CASE(3) BU_CASE(4) BU_CASE(5) BU_CASE(6) BU_CASE(7) BU_CASE(8) BU_CASE(9)
        BU_CASE(10) BU_CASE(11) BU_CASE(12) BU_CASE(13) BU_CASE(14) BU_CASE(15) BU_CASE(16) BU_CASE(17) BU_CASE(18)
#undef BU_CASE
    default: return BU_ST_BAD_MODE;  // 7-bit code 69 -> LUT value 19 (uastc.rs:329-341)
    }
}
