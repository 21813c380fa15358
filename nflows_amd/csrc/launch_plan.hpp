// Host-side launch planning of the per-layer kernels: tile sizes and grid sizes as plain functions of the problem and
// the device's CU count.  No HIP, no state, no side effects (tests/test_launch_plan_host.py compiles it for the host).
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace nfa {

constexpr int kBlock = 256;  // 4 wave64 per workgroup
constexpr int kWave = 64;
constexpr int kDefaultDynLds = 64 * 1024;  // dynamic LDS a launch may ask for without an opt-in
constexpr int kCuLds = 160 * 1024;         // LDS of one CU

inline int round_up4(int n) { return (n + 3) & ~3; }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ------------------------------------------------------------------------------------------
// Sample tiles: R whole samples per workgroup.

// about `lanes` items per tile (d_t items per sample; D where nothing is transformed), at least 1, at most the batch
inline int sample_rows(int lanes, int dt, int D, int64_t batch) {
    int R = dt > 0 ? lanes / dt : lanes / (D < lanes ? D : lanes);
    if (R < 1) R = 1;
    if ((int64_t)R > batch) R = (int)batch;
    return R;
}

struct SampleTile {
    int R = 0;       // samples per tile
    int C = 0;       // splines per chunk (0 = the whole tile's parameters at once)
    size_t lds = 0;  // bytes of the tile's LDS image
    bool ok = false;
};

// sample_rows(), halved until the image of lds_floats(r, chunk) floats fits `budget` bytes.  With P > 0 (parameters per
// spline: K1 and its backward) a single sample that does not fit streams its parameters through LDS in chunks of C
// splines, a multiple of kBlock, beside `chunk_fixed` bytes of everything else.  lds_floats may record the offsets it
// lays out: its last call is the one for the tile returned.  !ok: no tile fits, or one has 2^16 items or more.
template <typename F>
inline SampleTile plan_sample_tile(int lanes, int dt, int D, int64_t batch, size_t budget, F&& lds_floats, int P = 0,
                                   size_t chunk_fixed = 0) {
    SampleTile t;
    t.R = sample_rows(lanes, dt, D, batch);
    while (t.R > 1 && (size_t)lds_floats(t.R, 0) * 4 > budget) t.R >>= 1;
    if (P > 0 && t.R == 1 && (size_t)lds_floats(1, 0) * 4 > budget) {
        if (chunk_fixed + (size_t)kBlock * P * 4 > budget) return t;
        t.C = (int)((budget - chunk_fixed) / ((size_t)P * 4));
        t.C = (t.C / kBlock) * kBlock;
        if (t.C >= dt) t.C = 0;
    }
    t.lds = (size_t)lds_floats(t.R, t.C) * 4;
    t.ok = t.lds <= budget && (int64_t)t.R * dt < 65536 && (int64_t)t.R * D < 65536;
    return t;
}

// the layouts the pipelined K1 kernels take: whole float4s per sample, a tile within one pass of the workgroup
inline bool aligned_tile(int dt, int D, int P, int R, int64_t batch) {
    return dt > 0 && (dt * P) % 4 == 0 && D % 4 == 0 && R * dt <= kBlock && R * D <= 2 * kBlock && (int64_t)R <= batch;
}

// "full tiles through one kernel, the rows behind them through another": the rows of the first part
inline int64_t full_rows(int64_t batch, int64_t rows_per_tile) { return (batch / rows_per_tile) * rows_per_tile; }

// ------------------------------------------------------------------------------------------
// Element tiles: T elements per workgroup, kBlock halved down to `floor` until bytes(T) fits `budget`; 0 = none fits.
template <typename F>
inline int plan_element_tile(int floor, size_t budget, F&& bytes) {
    int T = kBlock;
    while (T > floor && (size_t)bytes(T) > budget) T >>= 1;
    return (size_t)bytes(T) <= budget ? T : 0;
}

// ------------------------------------------------------------------------------------------
// Persistent grids: the workgroups that are resident together, at most one per tile.
inline int64_t persistent_grid(int cus, int per_cu, int64_t tiles) {
    const int64_t g = (int64_t)cus * per_cu;
    return g > tiles ? tiles : g;
}
// ... where LDS decides residency: `lds` bytes of dynamic LDS (+ 256 of static arrays and granule) per workgroup, at
// most `cap` workgroups per CU
inline int64_t persistent_grid(int cus, size_t lds, int cap, int64_t tiles) {
    int per_cu = (int)((size_t)kCuLds / (lds + 256));
    if (per_cu > cap) per_cu = cap;
    if (per_cu < 1) per_cu = 1;
    return persistent_grid(cus, per_cu, tiles);
}

// ------------------------------------------------------------------------------------------
// K24 (householder.hip): a lane owns a row, the workgroup has R lanes (64, 128 or 256), the tile sits column-major in
// LDS with the odd row stride R + 1.  LDS image, in floats:
//   double logd[DP] | d[DP] | bias[DP] | c[chunk] | a[R] b[R] double cd[chunk] (backward only) | lad[4] | region |
//   tiles x DP (R + 1)
// DP = features rounded up to 16.  The region is shared by everything that is staged for one stage at a time: `chunk`
// reflection vectors, or the dense [DP, DP] image of the triangular factor.  tiles = 1 (forward) or 3 (backward: the
// rows in float64, two tiles' worth, and their gradients).
inline int hh_region_floats(int DP, int max_transforms, bool tri, int chunk) {
    const int k = max_transforms < chunk ? max_transforms : chunk;
    const int r = k * DP;
    return tri && DP * DP > r ? DP * DP : r;
}
inline size_t hh_lds_bytes(int DP, int region, int R, int tiles, int chunk) {
    return (size_t)4 * (4 * DP + chunk + (tiles > 1 ? 2 * R + 2 * chunk : 0) + 4 + region + tiles * DP * (R + 1));
}

struct HhTile {
    int R = 0;         // rows per workgroup = its lanes; 0: nothing fits
    size_t lds = 0;
    int64_t grid = 0;  // workgroups resident together, at most one per tile
};

// R: the most waves a CU can hold under its LDS (at most 8 workgroups, 16 waves), fewer lanes per workgroup on a tie
// (more workgroups: their load / compute / store phases overlap), then small enough that every CU gets a tile.
inline HhTile plan_hh_tile(int DP, int region, int tiles, int chunk, int max_R, int64_t batch, int cus) {
    HhTile t;
    int best = 0;
    for (int r = max_R; r >= kWave; r >>= 1) {
        const size_t lds = hh_lds_bytes(DP, region, r, tiles, chunk);
        if (lds + 256 > (size_t)kCuLds) continue;
        int blocks = (int)((size_t)kCuLds / (lds + 256));
        if (blocks > 8) blocks = 8;
        int waves = blocks * (r / kWave);
        if (waves > 16) waves = 16;
        if (waves > best || (waves == best && r < t.R)) {
            best = waves;
            t.R = r;
        }
    }
    if (best == 0) return t;
    while (t.R > kWave && (batch + t.R - 1) / t.R < (int64_t)cus) t.R >>= 1;
    t.lds = hh_lds_bytes(DP, region, t.R, tiles, chunk);
    t.grid = persistent_grid(cus, t.lds, 8, (batch + t.R - 1) / t.R);
    return t;
}

// ------------------------------------------------------------------------------------------
// Row sums of an elementwise map over [batch, n] rows (K18): who visits which element, and in which order a row's terms are
// added.  A function of (batch, n) only -- not of the device --, so the same shape gives the same bits everywhere.
//   n <= kRowSumTile  "rows": a workgroup takes `rows` whole rows, one contiguous range of rows * n <= kRowSumTile elements
//                     (a multiple of four rows where four fit: the range then starts on a float4 whatever n is); the terms
//                     of a row are added by `group` lanes (a power of two <= 64: lane g takes terms g, g + group, ... in
//                     order, the lanes are merged in a shuffle tree), about eight terms per lane.
//   n >  kRowSumTile  "pieces": a row is cut into `pieces` ranges of `piece` elements (a multiple of four; the last one
//                     shorter), one workgroup each: as many as fill kRowSumGroups workgroups, none shorter than half a tile.
//                     pieces > 1: the piece sums go to a float64 workspace [batch][pieces] and a second launch adds a
//                     row's pieces in piece order.
constexpr int kRowSumTile = 2048;     // elements of a workgroup's range in the rows regime: eight per lane
constexpr int kRowSumGroups = 1024;   // workgroups worth cutting rows for

struct RowSumPlan {
    int rows = 0;        // rows regime: rows per workgroup (0: pieces regime)
    int group = 1;       // rows regime: lanes that share a row's sum
    int pieces = 1;      // pieces regime: workgroups per row
    int64_t piece = 0;   // pieces regime: elements per piece
    int64_t groups = 0;  // workgroups of the launch
    bool vec4 = false;   // float4 lanes (given 16-byte aligned tensors)
};

inline RowSumPlan plan_row_sum(int64_t batch, int64_t n) {
    RowSumPlan p;
    if (batch < 1 || n < 1) return p;
    if (n <= kRowSumTile) {
        int R = (int)(kRowSumTile / n);
        if (R >= 4) R &= ~3;
        p.rows = R;
        int G = 1;
        while (G < kWave && (int64_t)G * 8 < n) G <<= 1;
        p.group = G;
        p.groups = (batch + R - 1) / R;
        p.vec4 = R % 4 == 0 || n % 4 == 0;
        return p;
    }
    int64_t S = (kRowSumGroups + batch - 1) / batch;
    const int64_t most = n / (kRowSumTile / 2);
    if (S > most) S = most;
    if (S < 1) S = 1;
    int64_t len = (n + S - 1) / S;
    len = (len + 3) & ~(int64_t)3;
    p.piece = len;
    p.pieces = (int)((n + len - 1) / len);
    p.groups = batch * p.pieces;
    p.vec4 = n % 4 == 0;
    return p;
}

// ------------------------------------------------------------------------------------------
// K20 "mog" (density.hip): a workgroup's range of elements comes from plan_row_sum(batch, features); an element's 3K
// parameters are contiguous, so the range's parameters are one contiguous range too and go through LDS in sub-tiles of
// T elements, T a power of two <= kBlock.  Beside the sub-tile the kernel holds kRowSumTile float64 terms and the waves'
// partial sums in static LDS; the whole stays within the 64 KB a launch gets without an opt-in.  Lane l always takes
// the elements l, l + kBlock, ... of the range, whatever T is: sub-tiling changes no summation order.
constexpr int kMogStaticLds = kRowSumTile * 8 + 1024;
// the LDS image of T elements: tile_load's 16-byte window around T * 3K floats
inline size_t mog_tile_bytes(int T, int K) { return ((size_t)T * 3 * K + 8) * 4; }
inline int plan_mog_tile(int K) {
    return plan_element_tile(1, (size_t)(kDefaultDynLds - kMogStaticLds), [K](int T) { return mog_tile_bytes(T, K); });
}

// ------------------------------------------------------------------------------------------
// K26 (rqs_resnet_f64.hip): a whole spline coupling layer in float64 on v_mfma_f64_16x16x4_f64.  A wave owns 16 rows,
// a workgroup's four waves a block of kF64Rows rows; the workgroups walk the row blocks persistently.
//
// The packed stream (doubles).  A matrix W [out, in] is held as the B fragments of its k-steps: k-step kk (4 values of
// `in`), column tile t (16 values of `out`), lane l hold W[16 t + (l & 15)][4 kk + (l >> 4)] at ((kk * nt + t) * 64 + l),
// zero past the matrix's own extents.  In order:
//   w_in      W_in  [H, di]           ks0 = ceil(di / 4) k-steps x NT = ceil(H / 16) tiles
//   w_blocks  per block W_0, W_1      ksh = HP / 4 k-steps x NT tiles each (HP = 16 NT)
//   w_final   W_f in chunks of F whole features (F P <= 128 columns; a multiple of four features where four fit, so
//             that 16 rows x F features fill whole waves): chunk c holds the rows [c F P, (c F + F_c) P) of W_f as ksh
//             k-steps x NTF = ceil(F P / 16) tiles -- the last chunk (F_last features) NTL = ceil(F_last P / 16) tiles
//   b_in      HP                      biases, zero-padded like the columns they belong to
//   b_blocks  per block b_0, b_1      HP each
//   b_final   per chunk 16 NTF (the last: 16 NTL)
constexpr int kF64Rows = 64;

struct F64LayerLayout {
    int HP = 0, NT = 0, ks0 = 0, ksh = 0;   // hidden width padded to 16, its tiles, k-steps of the initial / hidden Linears
    int F = 0, chunks = 0, NTF = 0, NTL = 0;
    int64_t w_in = 0, w_blocks = 0, w_final = 0, b_in = 0, b_blocks = 0, b_final = 0, total = 0;
};

inline F64LayerLayout f64_layer_layout(int di, int H, int num_blocks, int dt, int P) {
    F64LayerLayout l;
    l.NT = (H + 15) / 16;
    l.HP = 16 * l.NT;
    l.ks0 = (di + 3) / 4;
    l.ksh = l.HP / 4;
    int F = 128 / P;
    if (F >= 4) F &= ~3;
    if (F > dt) F = dt;
    l.F = F;
    l.chunks = (dt + F - 1) / F;
    const int last = dt - (l.chunks - 1) * F;
    l.NTF = (F * P + 15) / 16;
    l.NTL = (last * P + 15) / 16;
    const int64_t hidden = (int64_t)l.ksh * l.NT * 64;
    l.w_in = 0;
    l.w_blocks = (int64_t)l.ks0 * l.NT * 64;
    l.w_final = l.w_blocks + 2 * (int64_t)num_blocks * hidden;
    l.b_in = l.w_final + (int64_t)l.ksh * 64 * ((int64_t)(l.chunks - 1) * l.NTF + l.NTL);
    l.b_blocks = l.b_in + l.HP;
    l.b_final = l.b_blocks + 2 * (int64_t)num_blocks * l.HP;
    l.total = l.b_final + 16 * ((int64_t)(l.chunks - 1) * l.NTF + l.NTL);
    return l;
}

// LDS image of a workgroup, in doubles: per wave the activations [16][AS] (the next GEMM's A operand: AS = the widest k
// extent + 2, so that the 32 lanes of a ds_read_b64 pass fall into 32 different bank pairs) and a chunk's logits
// [16][LS], then two buffers of kc k-steps of the widest matrix.  kc: the most k-steps per buffer (8, 4, 2, 1) that fit
// the CU.  One workgroup per CU: the kernel's registers (two sets of accumulator tiles) leave room for one wave per SIMD.
struct F64LayerPlan {
    int AS = 0, LS = 0, kc = 0, max_nt = 0;
    size_t lds = 0;
    int64_t tiles = 0, grid = 0;
};

inline F64LayerPlan plan_f64_layer(const F64LayerLayout& l, int di, int64_t batch, int cus) {
    F64LayerPlan p;
    const int dip = 4 * l.ks0;
    p.AS = (l.HP > dip ? l.HP : dip) + 2;
    const int ntf = l.chunks > 1 && l.NTF > l.NTL ? l.NTF : l.NTL;
    p.LS = 16 * ntf + 1;
    p.max_nt = l.NT > ntf ? l.NT : ntf;
    const size_t fixed = (size_t)(kBlock / kWave) * 16 * (p.AS + p.LS) * 8;
    for (p.kc = 8; p.kc > 1; p.kc >>= 1)
        if (fixed + (size_t)2 * p.kc * p.max_nt * 64 * 8 + 256 <= (size_t)kCuLds) break;
    p.lds = fixed + (size_t)2 * p.kc * p.max_nt * 64 * 8;
    p.tiles = (batch + kF64Rows - 1) / kF64Rows;
    p.grid = persistent_grid(cus, p.lds, 1, p.tiles);
    return p;
}

}  // namespace nfa
