// conv_geom.hpp — tile tables, LDS stage arithmetic and size limits of the conv engines, stated ONCE: the host packer
// (model.cpp) decides with these functions what it packs, the launchers (conv_engine.hip.hpp, conv_sx_engine.hip.hpp, the
// fused pair kernels) take their geometry and their refusals from the same ones, so a conv that packs is a conv that launches.
// Host-side C++17, no HIP types (model.cpp stays HIP-free).
#pragma once
#include <cstddef>
#include <cstdlib>

namespace vitsmi {

// ---- budgets (bytes unless named otherwise)
constexpr int kLdsPerCu = 160 * 1024;
// (sx_publish_peak's four floats are static LDS: the dynamic part a kernel may ask for is the CU's LDS less that)
constexpr int kSxMaxDynLds = kLdsPerCu - 256;
constexpr int kLdsTwoPerCu = kLdsPerCu / 2 - 256;  // two workgroups per CU, each with that static part
constexpr int kDmaRound = 4096;                    // one LDS-DMA round of a workgroup: 256 cells of 16 bytes
constexpr int kSxStageMax = 12 * kDmaRound;        // an x stage of the sx engine: at most twelve rounds
constexpr int kSx16StageMax = 10 * kDmaRound;      // ... ten where the 16x16x32 packing is chosen: two workgroups per CU
constexpr int kSxRawStageCells = 768;              // raw-input staging: three cells per thread (two halves of LW cells)

// ---- f32 engine.  Tile configs: index -> (BM, BN)
//   0: 32x512   1: 64x256   2: 128x128 (long sequences)   3: 64x64   4: 32x128 (short sequences)
//   5: 32x64, the four waves split the reduction (KS = 4; token domain)
inline int conv_tile_m(int cfg) { return cfg == 2 ? 128 : ((cfg == 1 || cfg == 3) ? 64 : 32); }
inline int conv_tile_n(int cfg) {
    static const int n[6] = {512, 256, 128, 64, 128, 64};
    return cfg >= 0 && cfg < 6 ? n[cfg] : 128;
}

// largest pipeline stage (floats) a layer may use: 38 KiB (two workgroups per CU)
inline size_t conv_stage_capacity(int cfg) {
    static const long cap3 = [] {
        const char *e = std::getenv("VITSMI_STAGE_CAP_SMALL");  // tuning experiments only
        return e ? std::atol(e) : 4864l;
    }();
    if (cfg == 5) return 6144;  // (its workgroups hold >= 32 KiB for the partial tiles anyway: room for 32-channel chunks)
    return cfg <= 2 ? 9728 : size_t(cap3);
}

// One pipeline stage (x tile + A slab) of a conv on tile `cfg` with CK-channel chunks.  vec4: the 16-byte-DMA layout (rows
// padded to 16 bytes on both sides; never the smaller one), else 4-byte DMA.
struct ConvStage {
    int padLa, LW, xs_floats;
    size_t floats;     // x tile + A slab: what conv_stage_capacity() bounds
    int stage_floats;  // ... as laid out (whole 256-byte lines)
    size_t lds;        // two stages, bytes
    bool fits;
};
inline ConvStage conv_stage(int cfg, int K, int dil, int padL, int CK, bool vec4) {
    const int BN = conv_tile_n(cfg), BM = conv_tile_m(cfg), halo = (K - 1) * dil;
    ConvStage s;
    if (vec4) {
        s.padLa = (padL + 3) & ~3;
        s.LW = BN + s.padLa + ((halo - padL + 3) & ~3);
        s.xs_floats = (CK * s.LW + 1023) / 1024 * 1024;
    } else {
        s.padLa = padL;
        s.LW = BN + halo;
        s.xs_floats = (CK * s.LW + 255) / 256 * 256;
    }
    s.floats = size_t(s.xs_floats) + size_t(BM / 32) * size_t(K * CK / 8) * 256;
    s.stage_floats = int((s.floats + 63) / 64 * 64);
    s.lds = 2 * size_t(s.stage_floats) * sizeof(float);
    if (cfg == 5 && s.lds < size_t(4) * 2 * 16 * 64 * 4) s.lds = size_t(4) * 2 * 16 * 64 * 4;  // the four partial 32 x 64 tiles
    s.fits = s.floats <= conv_stage_capacity(cfg);
    return s;
}

// ---- split-operand (sx) engine.  Tile configs: index -> (BM, BN, waves WM x WN, blocks per wave MW x NW):
//   0: 128x256 (2x2 waves of 64x128)   1: 64x256 (2x2 waves of 32x128)   2: 32x256 (1x4 waves of 32x64)
// These are 256 columns wide: the weights of a step then serve 4 (2) block columns per register load.
//   3: 64x128 (2x2 waves of 32x64), run-time choice for short grids of 64-row layers (same packed weights as 1)
inline int sx_tile_m(int cfg) { return cfg == 0 ? 128 : ((cfg == 1 || cfg == 3) ? 64 : 32); }
inline int sx_tile_n(int cfg) { return cfg == 3 ? 128 : 256; }
// May the kernel of tile `run` read weights packed for tile `pack`?  Itself, or a shorter tile whose height divides the packed
// one (same products in the same order); the 64 x 128 tile exists for the 16x16x32 loop only.  These are the tiles conv_sx()
// may choose at run time for a packing.
inline bool sx_tile_reads(int pack, int run, bool s16) {
    return sx_tile_m(run) <= sx_tile_m(pack) && sx_tile_m(pack) % sx_tile_m(run) == 0 && (run != 3 || s16);
}

// The x stage of an sx conv on a tile BN columns wide.  planes: operand planes the mode reads (3 bf16, 2 fp16, 1 fp16);
// s16: the 16x16x32 loop (chunks of 32 channels: 4 channel groups x planes rows), else the 32x32x16 loop (chunks of 16
// channels: 2 channel-group halves x planes rows; needs K >= 3, pack_conv_sx pads narrower kernels).
struct SxStage {
    int LW, RS, xrows;
    unsigned x_bytes;  // one stage, padded to whole DMA rounds so that every wave issues the same count
    size_t lds;
    bool fits;         // the mode exists on this loop and the stage is within the engine's limits
    bool raw_ok;       // ... and within those of raw-input staging
    size_t row_bytes() const { return size_t(xrows) * RS * 16; }
    size_t packed_bytes() const { return size_t(xrows) * LW * 16; }  // with RS = LW (rows not spread for the LDS banks)
};
inline SxStage sx_stage(int BN, int K, int dil, int planes, bool s16) {
    const auto rounds = [](size_t b) { return (b + kDmaRound - 1) / kDmaRound * kDmaRound; };
    SxStage s;
    const long long lw = BN + (long long)(K - 1) * dil;
    s.LW = lw < (1 << 20) ? int(lw) : 1 << 20;  // (refused far below that; an absurd dilation in a file must not overflow)
    s.RS = s.LW;
    s.xrows = (s16 ? 4 : 2) * planes;
    if (s16) {
        // rows 16 cells apart modulo 16: the ds_read_b128 of a B fragment (lanes 16 apart = the next channel group) is then
        // free of bank conflicts; where that does not fit two workgroups per CU the rows stay packed (mild conflicts)
        // (two workgroups per CU = 80 KiB each, all of it dynamic: the 16x16x32 kernels have no static LDS)
        const size_t rs16 = size_t(s.LW + 15) / 16 * 16, b16 = s.xrows * rs16 * 16;
        if (rounds(b16) + b16 <= size_t(kLdsPerCu / 2)) s.RS = int(rs16);
    }
    s.x_bytes = unsigned(rounds(s.row_bytes()));
    // two x stages; the weights never touch LDS.  (16x16x32: the second stage ends with its last row - the DMA rounds are
    // whole 4 KiB but lanes past the last row are masked off - which keeps the 50-cell halo of a k = 11, dilation 5 conv
    // inside 80 KiB)
    s.lds = s16 ? size_t(s.x_bytes) + s.row_bytes() : 2 * size_t(s.x_bytes);
    s.fits = (s16 ? planes <= 2 : (planes >= 2 && K >= 3)) && s.x_bytes <= unsigned(kSxStageMax) && s.lds <= size_t(kSxMaxDynLds);
    s.raw_ok = 2 * s.LW <= kSxRawStageCells;
    return s;
}

}  // namespace vitsmi
