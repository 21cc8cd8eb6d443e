// kernels_join.hip -- the sketch-on-sketch join (szg_index_neighbors): the queries are stored
// rows, so their 8-bit sketch rows are resident already and lie in the tiled layout [tile][step][row & 15][piece & 3],
// which is the operand layout of v_mfma_i32_16x16x64_i8 on BOTH sides.  One digit plane, one MFMA per (query tile, row
// tile, 64-byte step), exact int32 sums, no query preparation.
//
// Work split.  A block owns a query block of QB = 16 NW query rows (NW waves, one query tile of 16 rows each) and a slice
// of the shard's row tiles; the grid is (query blocks) x (slices),
// block b = query block b % query_blocks of slice b / query_blocks.  The block stages the slice's row tiles through LDS in
// a double buffer, in units of up to kJoinStageSteps whole 1 KiB step lines of one tile: every thread loads its 16-byte
// share of the next unit from HBM (non-temporal) while the waves multiply the current one, all NW waves read their B
// operands from LDS -- one HBM read of a row tile serves QB queries.  A wave's own query tile, the A operand, stays in
// registers where the rows have at most 16 steps (AREG: 64 VGPRs, and a unit is a whole tile); longer rows keep the
// block's QB query rows in LDS behind the stages.  Both operands are the stored bytes xor 0x80, i.e. v' = v - 128 as
// signed bytes (the element is n = 2 v' + 1), so with P = sum a' b', S1 = sum v' and S2 = sum v'^2 of a row (JoinRowStat,
// join_row_stats_kernel):
//   Euclid   |n_a - n_b|^2 = 4 (S2_a + S2_b - 2 P)                     an exact int32, rounded once to the float32 key
//   cosine   n_a . n_b     = 4 P + 2 (S1_a + S1_b) + dim               an exact int32; key = -float(dot) * rinv_a * rinv_b
// static_assert below: both stay inside int32 up to 4 096 dimensions.
//
// Selection.  After a tile lane (c, t) holds the dots of queries 4 c .. 4 c + 3 of the wave's tile against row t -- the
// matrix sweep's accumulator layout -- so the lists are its row lists (RowList, device_lists.h; rowlists_offer, row_offer.h): four
// register pairs per lane, list length m <= 16, worst-key pre-filter, crowded tiles merged whole.  A wave's lists are
// the block's: it alone scores its queries.  Out: lists[(query * slices + slice) * m + j], sorted, kInvalidCand-padded;
// launch_merge_short merges the slices and leaves the drop bound.
//
// MASKED: rows are eligible by live AND allow (one mask for all queries); tiles without an eligible row are not loaded
// (mask_tiles.h).  The unmasked form has no mask loads.
#ifndef SZG_MX_NO_SLP
#error "compile with -fno-slp-vectorize -DSZG_MX_NO_SLP (the row lists' scalar wave masks: see the Makefile)"
#endif
#include "join_plan.h"
#include "mask_tiles.h"
#include "row_offer.h"

namespace szg {

namespace {

typedef int v4i32 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

static_assert(127ll * 128 * kJoinMaxDim * 4 + 2ll * 2 * 128 * kJoinMaxDim + kJoinMaxDim < (1ll << 31),
              "cosine: 4 P + 2 (S1a + S1b) + dim fits int32");
static_assert(4ll * 255 * 255 * kJoinMaxDim < (1ll << 31), "Euclid: 4 sum (a' - b')^2 fits int32");
static_assert(128ll * 128 * kJoinMaxDim < (1ll << 31), "|P| and S2 fit int32");

__device__ __forceinline__ v4i32 flip(u32x4 v)
{
    return v4i32{(int)(v.x ^ 0x80808080u), (int)(v.y ^ 0x80808080u), (int)(v.z ^ 0x80808080u), (int)(v.w ^ 0x80808080u)};
}

__device__ __forceinline__ int sum4(uint32_t w, int *sq)
{
    int s = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int v = (int)((w >> (8 * b)) & 0xFFu) - 128;
        s += v;
        *sq += v * v;
    }
    return s;
}

// S1, S2 and 1 / |n| of tiled 8-bit rows [0, n_rows) of `steps` whole steps: one thread per row
__global__ __launch_bounds__(256) void join_row_stats_kernel(const uint8_t *rows, uint32_t n_rows, uint32_t steps, int dim,
                                                             JoinRowStat *out)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rows) return;
    const uint8_t *p = rows + (size_t)(r >> 4) * steps * 1024 + (size_t)(r & 15) * 64;
    int s1 = 0, s2 = 0;
    for (uint32_t st = 0; st < steps; st++) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u32x4 v = *reinterpret_cast<const u32x4 *>(p + (size_t)st * 1024 + j * 16);
            s1 += sum4(v.x, &s2) + sum4(v.y, &s2) + sum4(v.z, &s2) + sum4(v.w, &s2);
        }
    }
    const double n2 = 4.0 * ((double)s2 + (double)s1) + (double)dim;  // sum (2 v' + 1)^2 >= dim
    out[r] = JoinRowStat{s1, s2, (float)(1.0 / sqrt(n2)), 0};
}

template <int METRIC, int NW, bool AREG, bool MASKED>
__global__ __launch_bounds__(64 * NW) void join_kernel(const JoinArgs a)
{
    extern __shared__ __align__(16) uint8_t smem[];
    constexpr int T = 64 * NW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane >> 4, t = lane & 15;
    const uint32_t steps = a.steps;
    const uint32_t sc = steps < (uint32_t)kJoinStageSteps ? steps : (uint32_t)kJoinStageSteps;  // steps per unit
    const uint32_t chunks = (steps + sc - 1) / sc;
    const uint32_t stage_bytes = sc * 1024u;
    uint8_t *stage[2] = {smem, smem + stage_bytes};
    const uint32_t lane_off = (uint32_t)t * 64u + (uint32_t)c * 16u;  // this lane's 16 bytes of a step line
    const uint32_t qblock = blockIdx.x % a.query_blocks, slice = blockIdx.x / a.query_blocks;
    const uint32_t qtile = qblock * NW + wave;                        // the wave's query tile of the batch
    const uint32_t q_tiles = (a.n_queries + 15u) >> 4;
    const bool wave_on = qtile < q_tiles;
    const uint8_t *qsrc = a.qtiles + (size_t)(wave_on ? qtile : 0) * steps * 1024;

    // the A operand: registers (AREG: steps <= 16), else the block's query rows in LDS behind the stages
    [[maybe_unused]] v4i32 areg[16];
    [[maybe_unused]] uint8_t *alds = smem + 2 * stage_bytes + (size_t)wave * steps * 1024;
    if constexpr (AREG) {
#pragma unroll
        for (int st = 0; st < 16; st++)
            areg[st] = (uint32_t)st < steps ? flip(*reinterpret_cast<const u32x4 *>(qsrc + (size_t)st * 1024 + lane_off))
                                            : v4i32{0, 0, 0, 0};
    } else {
        for (uint32_t st = 0; st < steps; st++)
            *reinterpret_cast<v4i32 *>(alds + (size_t)st * 1024 + lane_off) =
                flip(*reinterpret_cast<const u32x4 *>(qsrc + (size_t)st * 1024 + lane_off));
    }
    // this lane's four queries: 16 qtile + 4 c + r
    bool qlive[4];
    int qs1[4], qs2[4];
    float qrinv[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t q = qtile * 16u + (uint32_t)c * 4u + (uint32_t)r;
        qlive[r] = q < a.n_queries;
        const JoinRowStat s = a.q_stat[qlive[r] ? q : 0];
        qs1[r] = s.s1, qs2[r] = s.s2, qrinv[r] = s.rinv;
    }
    RowList rls[4];
    float wk[4];
#pragma unroll
    for (int r = 0; r < 4; r++) rls[r].init(), wk[r] = __builtin_inff();

    const uint64_t n_tiles = ((uint64_t)a.n_rows + 15) >> 4;
    const uint64_t tile_lo = (uint64_t)slice * a.tiles_per_slice;
    const uint64_t tile_hi = tile_lo + a.tiles_per_slice < n_tiles ? tile_lo + a.tiles_per_slice : n_tiles;
    auto next_tile = [&](uint64_t from) -> uint64_t {
        if constexpr (MASKED) return mask_next_tile(a.live, a.allow, from, 1, tile_hi).tile;
        return from < tile_hi ? from : tile_hi;
    };
    // a unit: steps [chunk sc, chunk sc + n) of one tile, 64 n pieces of 16 bytes, thread tid takes pieces tid, tid + T, ...
    constexpr int kLoads = (kJoinStageSteps * 64 + T - 1) / T;
    u32x4 ring[kLoads];
    auto unit_steps = [&](uint32_t chunk) { return steps - chunk * sc < sc ? steps - chunk * sc : sc; };
    auto load_unit = [&](uint64_t tile, uint32_t chunk) {
        const uint8_t *src = a.rows + ((size_t)tile * steps + (size_t)chunk * sc) * 1024;
        const uint32_t pieces = unit_steps(chunk) * 64u;
#pragma unroll
        for (int i = 0; i < kLoads; i++) {
            const uint32_t p = (uint32_t)tid + (uint32_t)i * T;
            if (p < pieces) ring[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(src + (size_t)p * 16));
        }
    };
    auto store_unit = [&](uint8_t *dst, uint32_t chunk) {
        const uint32_t pieces = unit_steps(chunk) * 64u;
#pragma unroll
        for (int i = 0; i < kLoads; i++) {
            const uint32_t p = (uint32_t)tid + (uint32_t)i * T;
            if (p < pieces) *reinterpret_cast<v4i32 *>(dst + (size_t)p * 16) = flip(ring[i]);
        }
    };

    uint64_t tile = next_tile(tile_lo);
    uint32_t chunk = 0;
    if (tile < tile_hi) {
        load_unit(tile, 0);
        store_unit(stage[0], 0);
    }
    __syncthreads();  // (the A rows in LDS too)
    v4i32 acc = {0, 0, 0, 0};
    for (uint32_t u = 0; tile < tile_hi; u++) {
        // the unit behind this one
        uint64_t tile2 = tile;
        uint32_t chunk2 = chunk + 1;
        if (chunk2 == chunks) chunk2 = 0, tile2 = next_tile(tile + 1);
        if (tile2 < tile_hi) load_unit(tile2, chunk2);
        const bool last = chunk + 1 == chunks;
        JoinRowStat rs{0, 0, 0.0f, 0};
        const uint64_t row = tile * 16 + (uint64_t)t;
        const bool row_ok = row < a.n_rows;
        if (last && row_ok) rs = a.row_stat[row];
        // multiply
        const uint8_t *b = stage[u & 1] + lane_off;
        const uint32_t n = unit_steps(chunk);
        if (wave_on) {
            if constexpr (AREG) {
#pragma unroll
                for (int st = 0; st < 16; st++)
                    if ((uint32_t)st < n)
                        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(areg[st], *reinterpret_cast<const v4i32 *>(b + (size_t)st * 1024),
                                                                    acc, 0, 0, 0);
            } else {
                const uint8_t *ap = alds + (size_t)chunk * sc * 1024 + lane_off;
                for (uint32_t st = 0; st < n; st++)
                    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const v4i32 *>(ap + (size_t)st * 1024),
                                                                *reinterpret_cast<const v4i32 *>(b + (size_t)st * 1024), acc, 0, 0, 0);
            }
        }
        if (last && wave_on) {
            // the tile is done: lane (c, t) holds queries 4 c + r against row t
            bool elig = row_ok;
            if constexpr (MASKED) {
                uint32_t sl = 0xFFFFu;
                if (a.live) sl &= mask_tile_slice(a.live, tile);
                if (a.allow) sl &= mask_tile_slice(a.allow, tile);
                elig = elig && ((sl >> t) & 1u);
            }
            uint32_t uk[4];
            bool pass[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float key;
                if constexpr (METRIC == kCosine) {
                    const int dot = 4 * acc[r] + 2 * (qs1[r] + rs.s1) + a.dim;
                    key = -((float)dot * qrinv[r]) * rs.rinv;
                } else {
                    key = (float)(4 * (qs2[r] + rs.s2 - 2 * acc[r]));
                }
                uk[r] = ordered_key(key);
                pass[r] = elig && qlive[r] && !(key > wk[r]);
            }
            rowlists_offer<4>(rls, pass, uk, (uint32_t)(tile * 16), (uint32_t)row, lane, a.m, kBulkMin, wk);
        }
        if (last) acc = v4i32{0, 0, 0, 0};
        if (tile2 < tile_hi) store_unit(stage[(u + 1) & 1], chunk2);
        __syncthreads();
        tile = tile2, chunk = chunk2;
    }
    // lane (c, j) holds entry j of query 4 c + r's list
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t q = qtile * 16u + (uint32_t)c * 4u + (uint32_t)r;
        if (wave_on && qlive[r] && t < a.m) a.lists[((size_t)q * a.slices + slice) * a.m + t] = rls[r].mine;
    }
}

template <int METRIC, int NW, bool AREG>
hipError_t launch_join_m(const JoinArgs &a, const JoinPlan &p, bool masked, hipStream_t stream)
{
    const int grid = p.query_blocks * p.slices, block = 64 * NW;
    if (masked) return launch_mxl<join_kernel<METRIC, NW, AREG, true>>(a, grid, block, p.lds_bytes, stream);
    return launch_mxl<join_kernel<METRIC, NW, AREG, false>>(a, grid, block, p.lds_bytes, stream);
}
template <int METRIC>
hipError_t launch_join_q(const JoinArgs &a, const JoinPlan &p, bool masked, hipStream_t stream)
{
    switch (p.qb) {
    case 64: return p.areg ? launch_join_m<METRIC, 4, true>(a, p, masked, stream) : launch_join_m<METRIC, 4, false>(a, p, masked, stream);
    case 32: return launch_join_m<METRIC, 2, false>(a, p, masked, stream);
    case 16: return launch_join_m<METRIC, 1, false>(a, p, masked, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_join_row_stats(const uint8_t *rows, uint32_t n_rows, uint32_t steps, int dim, JoinRowStat *out, hipStream_t stream)
{
    if (n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(join_row_stats_kernel, dim3((n_rows + 255u) / 256u), dim3(256), 0, stream, rows, n_rows, steps, dim, out);
    return hipGetLastError();
}

// The last check before the kernel: the launch is exactly one that join_plan made for these rows -- anything else would
// read or write out of bounds.
hipError_t launch_join(int metric, const JoinArgs &a, const JoinPlan &p, hipStream_t stream)
{
    const bool masked = a.live != nullptr || a.allow != nullptr;
    const uint64_t n_tiles = ((uint64_t)a.n_rows + 15) >> 4;
    if (!p.served || a.n_rows == 0 || a.n_queries == 0 || a.steps < 1 || a.steps * 64u != (uint32_t)a.dim || a.dim > kJoinMaxDim ||
        a.m < 1 || a.m > kRowListMax || a.m != p.m || (int)a.tiles_per_slice != p.tiles_per_slice || (int)a.query_blocks != p.query_blocks ||
        (int)a.slices != p.slices ||
        (uint64_t)p.slices * a.tiles_per_slice < n_tiles || (uint64_t)p.query_blocks * p.qb < a.n_queries ||
        p.lds_bytes != join_lds_bytes(a.dim, p.qb) || p.lds_bytes > kLongLdsCu || (p.areg != 0) != join_areg(a.dim, p.qb) ||
        (masked != (p.masked != 0)))
        return hipErrorInvalidValue;
    return metric == kCosine ? launch_join_q<kCosine>(a, p, masked, stream) : launch_join_q<kEuclidean>(a, p, masked, stream);
}

}  // namespace szg
