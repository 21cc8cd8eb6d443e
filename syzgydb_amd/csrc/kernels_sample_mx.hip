// kernels_sample_mx.hip -- the sample pass of a top-k search of large k through the sketch (option sketch_topk_collect;
// DESIGN.md 4.5 item 16; sample_plan.h has its arithmetic, scan_sketch_topk.cpp its caller).
//
// sample_mx_kernel scores a strided sample of a sketch shard on the matrix cores: every stride-th tile of 16 tiled 8-bit
// rows against the 16 (NB = 1) or 32 (NB = 2) two-plane queries of the launch.  The operands are scan_mx_kernel's
// (kernels_scan_mx.hip): the B operand of a 64-byte step is the row bytes as loaded (lane = chunk * 16 + row) xor
// 0x80808080, the A operand the same elements of a digit plane of 16 queries (lane = chunk * 16 + query) from the image
// in LDS; one v_mfma_i32_16x16x64_i8 per plane, block and step.  After a tile lane (c, t) holds the exact plane sums M, L
// of queries 16 b + 4 c + r against row t.  The key chain from there is that kernel's, operation by operation -- SHAPED
// says which of its two conversions the collect sweep of the same rows takes (rows of 12 or 6 steps: the integer
// combine (float)(128 M + L); any other: fmaf(128, float(M), float(L))) -- so a (query, row) pair gets the key the
// collect form gives it, bit for bit, and key_eps' two-plane integer bound holds for it unchanged.
// There are no lists: every scored pair writes its ordered 32-bit key to keys[query][16 j + t] (sample tile j, row t),
// kSampleNoKey where the row does not exist, is dead (live bits) or is outside the query's mask (a tile is one aligned
// 16-bit slice of a mask word, mask_tiles.h; one mask for all queries -- allow_stride 0 -- or one per query).
// The sample is a sixteenth to a half of the rows and a tile's loads go out four steps at a time, without the ring the
// sweep kernels keep: the pass is short beside the collect sweep that follows it.
//
// sample_select_kernel, one block per query: the key of a given rank among the query's sample keys and the number of
// valid ones -- a radix select over the ordered keys, four passes of eight bits with a 256-bin histogram in LDS, no sort.
// Fewer valid keys than the rank: kSampleNoKey.
//
// Resources (hipcc --offload-arch=gfx950 -O3, scripts/kernel_resources.sh sample): no kernel of this file uses scratch.
//   sample_mx_kernel NB = 1: 70 (cosine) / 74 (Euclid) VGPRs, 63 SGPRs, LDS 2 KiB per step + 192 bytes
//   (768 dimensions: 24.2 KiB); NB = 2: 102 / 106 VGPRs, 72 SGPRs, LDS 4 KiB per step + 384 bytes (48.4 KiB); launch bound
//   256 threads, two blocks per CU.  sample_select_kernel: 10 VGPRs, 256 threads, 1 KiB of histogram and four words of LDS.
#include "kernels.h"
#include "mask_tiles.h"

namespace szg {

namespace {

typedef int v4i32 __attribute__((ext_vector_type(4)));
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;

constexpr uint32_t kNoKey = 0xFFFFFFFFu;

template <int METRIC, bool SHAPED, int NB>
__global__ __launch_bounds__(256, 2) void sample_mx_kernel(const SampleArgs s)
{
    const ScanArgs &a = s.a;
    constexpr int kQ = kMatrixQueries * NB;  // queries of the launch's one group
    constexpr int NS = 4 * NB;               // slots (queries) per lane
    extern __shared__ __align__(16) uint8_t smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwaves = blockDim.x >> 6;
    const int steps = (int)a.steps;
    const int n16 = steps * 2 * 64;  // 16-byte words of a block's image: [step][plane m, l][chunk * 16 + query]

    // LDS: the image [block] | qscale, qconst, qnorm2 [16 NB]
    uint4 *image = reinterpret_cast<uint4 *>(smem);
    float *qtab = reinterpret_cast<float *>(smem + (size_t)NB * n16 * 16);
    // column x holds query min(x, n_queries - 1): the idle columns score the last query again and write nothing
    for (int i0 = tid; i0 < NB * n16; i0 += blockDim.x) {
        const int blk = NB == 1 ? 0 : (i0 >= n16 ? 1 : 0), i = i0 - blk * n16;
        const int x = i & 15, chunk = (i >> 4) & 3, p = (i >> 6) & 1, st = i >> 7;
        const int q = min(blk * kMatrixQueries + x, a.n_queries - 1);
        // (the staged query is [plane h, m, l][piece]: the all-zero h plane stays behind)
        const uint4 *src = reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(a.query) + (size_t)q * a.query_stride) +
                           (size_t)(1 + p) * a.map.r16 + (st * 4 + chunk);
        image[i0] = *src;
    }
    if (tid < kQ) {
        const int q = min(tid, a.n_queries - 1);
        qtab[tid] = a.qscale[q];
        qtab[kQ + tid] = a.qconst[q];
        qtab[2 * kQ + tid] = a.qnorm2[q];
    }
    __syncthreads();

    const int trow = lane & 15;
    const int c = lane >> 4;
    const RowLayout lay{a.pitch, a.tiled, a.steps};
    const uint64_t last_row = a.n_rows ? (uint64_t)a.n_rows - 1 : 0;
    float qsv[NS], qcv[NS], qnv[NS];
    int qof[NS];
#pragma unroll
    for (int r = 0; r < NS; r++) {
        const int x = (r >> 2) * kMatrixQueries + c * 4 + (r & 3);  // this slot's column, and its query
        qof[r] = x;
        qsv[r] = qtab[x];
        qcv[r] = qtab[kQ + x];
        qnv[r] = qtab[2 * kQ + x];
    }
    const v4i32 *qimg = reinterpret_cast<const v4i32 *>(smem) + lane;
    const bool per_query = a.allow_bits != nullptr && a.allow_stride != 0;

    for (uint64_t j = (uint64_t)blockIdx.x * nwaves + wave; j < s.tiles; j += (uint64_t)gridDim.x * nwaves) {
        const uint64_t tile = j * s.stride;  // (< ceil(n_rows / 16): the launcher checks tiles against the rows)
        const uint64_t row = tile * 16 + trow;
        const bool row_ok = row < a.n_rows;
        // (a row past the end of the last tile: a valid row, read and discarded)
        const uint8_t *ptr = a.rows + piece_offset(lay, min(row, last_row), (uint32_t)c);
        const float norm = a.row_norm[min(row, last_row)];
        v4i32 accM[NB], accL[NB];
#pragma unroll
        for (int b = 0; b < NB; b++) accM[b] = accL[b] = v4i32{0, 0, 0, 0};
        for (int st0 = 0; st0 < steps; st0 += 4) {
            u32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; u++)  // (past the row's last step: its last step again, loaded and not multiplied)
                v[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(ptr + (size_t)min(st0 + u, steps - 1) * 1024));
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int st = st0 + u;
                if (st < steps) {  // (wave-uniform)
                    v4i32 bop;
                    bop[0] = (int)(v[u].x ^ 0x80808080u);
                    bop[1] = (int)(v[u].y ^ 0x80808080u);
                    bop[2] = (int)(v[u].z ^ 0x80808080u);
                    bop[3] = (int)(v[u].w ^ 0x80808080u);
#pragma unroll
                    for (int b = 0; b < NB; b++) {
                        const v4i32 am = qimg[((b * steps + st) * 2 + 0) * 64];
                        const v4i32 al = qimg[((b * steps + st) * 2 + 1) * 64];
                        accM[b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(am, bop, accM[b], 0, 0, 0);
                        accL[b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bop, accL[b], 0, 0, 0);
                    }
                }
            }
        }
        // eligibility of this lane's row: the tile's slice of the live words and of the mask every query shares
        uint32_t shared_sl = 0xFFFFu;
        if (a.live_bits) shared_sl &= mask_tile_slice(a.live_bits, tile);
        if (a.allow_bits && !per_query) shared_sl &= mask_tile_slice(a.allow_bits, tile);
        const bool shared_ok = row_ok && ((shared_sl >> trow) & 1u) != 0;
        const float inv = __frsqrt_rn(norm);
#pragma unroll
        for (int r = 0; r < NS; r++) {
            // scan_mx_kernel's finish_tile, operation by operation
            float dot;
            if constexpr (SHAPED) dot = (float)(accM[r >> 2][r & 3] * 128 + accL[r >> 2][r & 3]);
            else dot = fmaf(128.0f, (float)accM[r >> 2][r & 3], (float)accL[r >> 2][r & 3]);
            const float d2 = fmaf(2.0f, dot, qcv[r]);  // sum Q n
            float k_;
            if constexpr (METRIC == kCosine) k_ = -(d2 * qsv[r]) * inv;
            else k_ = fmaf(-2.0f * qsv[r], d2, qnv[r] + norm);
            k_ = fminf(k_, 3.0e38f);
            const int q = qof[r];
            if (q >= a.n_queries) continue;  // an idle column
            bool ok = shared_ok;
            if (per_query) ok = ok && ((mask_tile_slice(a.allow_bits + (size_t)q * a.allow_stride, tile) >> trow) & 1u) != 0;
            s.keys[(size_t)q * s.slots + j * 16 + trow] = ok ? ordered_key(k_) : kNoKey;
        }
    }
}

__global__ __launch_bounds__(256) void sample_select_kernel(const SampleSelectArgs s)
{
    __shared__ uint32_t hist[256];
    __shared__ uint32_t ctl[4];  // no-key slots | the bin found | the rank left inside it
    const int tid = threadIdx.x;
    const uint32_t q = blockIdx.x;
    const uint32_t *keys = s.keys + (size_t)q * s.slots;
    uint32_t rank = s.rank[q];  // 1-based
    uint32_t prefix = 0, mask = 0;
    if (tid == 0) ctl[0] = 0;
    for (int pass = 0; pass < 4; pass++) {
        const int shift = 24 - 8 * pass;
        hist[tid] = 0;
        __syncthreads();
        uint32_t nokey = 0;
        for (uint32_t i = tid; i < s.slots; i += 256) {
            const uint32_t k = keys[i];
            nokey += k == kNoKey ? 1u : 0u;
            if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
        }
        if (pass == 0 && nokey) atomicAdd(&ctl[0], nokey);
        __syncthreads();
        if (pass == 0) {
            // (a valid key is clamped to 3e38: it orders below kSampleNoKey, so the rank-th smallest slot is a valid key
            // exactly when at least `rank` slots are valid)
            const uint32_t valid = s.slots - ctl[0];
            if (rank < 1 || valid < rank) {  // (block-uniform)
                if (tid == 0) {
                    s.out[2 * q] = kNoKey;
                    s.out[2 * q + 1] = valid;
                }
                return;
            }
            if (tid == 0) s.out[2 * q + 1] = valid;
        }
        if (tid == 0) {
            uint32_t cum = 0, b = 0;
            for (; b < 255; b++) {
                if (cum + hist[b] >= rank) break;
                cum += hist[b];
            }
            ctl[1] = b;
            ctl[2] = rank - cum;
        }
        __syncthreads();
        prefix |= ctl[1] << shift;
        mask |= 255u << shift;
        rank = ctl[2];
        __syncthreads();  // (ctl and hist are written again by the next pass)
    }
    if (tid == 0) s.out[2 * q] = prefix;
}

template <int METRIC>
hipError_t launch_sample_metric(const SampleArgs &s, bool shaped, int nb, int grid, int block, size_t lds, hipStream_t stream)
{
    if (nb == 2) {
        if (shaped) hipLaunchKernelGGL((sample_mx_kernel<METRIC, true, 2>), dim3(grid), dim3(block), lds, stream, s);
        else hipLaunchKernelGGL((sample_mx_kernel<METRIC, false, 2>), dim3(grid), dim3(block), lds, stream, s);
    } else {
        if (shaped) hipLaunchKernelGGL((sample_mx_kernel<METRIC, true, 1>), dim3(grid), dim3(block), lds, stream, s);
        else hipLaunchKernelGGL((sample_mx_kernel<METRIC, false, 1>), dim3(grid), dim3(block), lds, stream, s);
    }
    return hipGetLastError();
}

}  // namespace

size_t sample_mx_lds_bytes(uint32_t steps, int nb)
{
    return (size_t)nb * steps * 2 * 64 * 16 + (size_t)3 * kMatrixQueries * nb * sizeof(float);
}

hipError_t launch_sample_mx(int metric, const SampleArgs &s, int nb, int grid, int block, hipStream_t stream)
{
    const ScanArgs &a = s.a;
    // (what the kernel takes for granted: a launch that does not meet it must not reach it)
    if ((nb != 1 && nb != 2) || !a.tiled || a.steps == 0 || (int)a.steps * 4 != a.map.r16 || a.planes != 2 || !a.row_norm ||
        !a.rows || !a.query || !s.keys || a.n_rows == 0 || a.n_queries < 1 || a.n_queries > kMatrixQueries * nb ||
        block < 64 || block > 256 || block % 64 || grid < 1 || s.stride < 1)
        return hipErrorInvalidValue;
    const uint64_t n_tiles = ((uint64_t)a.n_rows + 15) / 16;
    if (s.tiles != (n_tiles + s.stride - 1) / s.stride || (uint64_t)s.slots != (uint64_t)s.tiles * 16) return hipErrorInvalidValue;
    const size_t lds = sample_mx_lds_bytes(a.steps, nb);
    if (lds > 64u * 1024u) return hipErrorInvalidValue;
    // the conversion the collect sweep of these rows takes (kernels_scan_mx.hip: the shaped kernels combine as integers)
    const bool shaped = matrix_steps_form((int)a.steps) != 0;
    return metric == kCosine ? launch_sample_metric<kCosine>(s, shaped, nb, grid, block, lds, stream)
                             : launch_sample_metric<kEuclidean>(s, shaped, nb, grid, block, lds, stream);
}

hipError_t launch_sample_select(const SampleSelectArgs &s, int n_queries, hipStream_t stream)
{
    if (!s.keys || !s.out || s.slots == 0 || n_queries < 1 || n_queries > kMatrixWideQueries) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_select_kernel, dim3(n_queries), dim3(256), 0, stream, s);
    return hipGetLastError();
}

}  // namespace szg
