// kernels_column.hip -- resident metadata columns (szg_column, scan_column.cpp): a comparison of ONE shard's part of a
// column against a constant, written straight into the words of a filter mask (kernels_mask.hip has the layout: 16-byte
// pairs of words, bits at positions >= n_rows stored as 0).
//
// One wave step covers 128 rows = one pair: lane l holds elements base + l and base + 64 + l (two contiguous wave loads),
// two ballots give the pair's words, lane 0 stores them with one 16-byte store.  kSteps steps of a wave are loaded
// before the first is used.  No element at a position >= n_rows is loaded.  Plain C++ and vector memory operations only.
// A text column's element is a row's 8-byte reference into a byte heap that the predicate then reads (column_str.h;
// column_dfa.h for the walk of a byte automaton).
#include "kernels.h"
#include "column_str.h"
#include "column_dfa.h"

namespace szg {

namespace {

constexpr int kSteps = 4;  // wave steps whose loads are in flight together

// IEEE comparisons, as Go's == / < on float64 (query/compiler.go:175, :288-303): -0.0 == 0.0, NaN only passes NE
struct CmpF64 {
    using T = double;
    static constexpr bool kLoads = true;
    int op;
    double c;
    __device__ void init() {}
    __device__ bool operator()(double v) const
    {
        switch (op) {
        case 0: return v == c;
        case 1: return v != c;
        case 2: return v < c;
        case 3: return v <= c;
        case 4: return v > c;
        default: return v >= c;
        }
    }
};

// membership in up to kColumnInMax sorted constants (no NaN among them), held in LDS: a binary search per lane
struct InF64 {
    using T = double;
    static constexpr bool kLoads = true;
    const double *vals;  // device, ascending
    uint32_t n;
    const double *lds;
    __device__ void init()
    {
        __shared__ double s[kColumnInMax];
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) s[i] = vals[i];
        __syncthreads();
        lds = s;
    }
    __device__ bool operator()(double v) const
    {
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (lds[mid] < v) lo = mid + 1;
            else hi = mid;
        }
        return lo < n && lds[lo] == v;   // (a NaN ends at lo == 0 and equals nothing)
    }
};

// a bit test in a bitmap over codes; a code >= n_codes fails
struct CodeBits {
    using T = uint32_t;
    static constexpr bool kLoads = true;
    const uint64_t *bits;  // device, ceil(n_codes / 64) words
    uint32_t n_codes;
    __device__ void init() {}
    __device__ bool operator()(uint32_t code) const
    {
        if (code >= n_codes) return false;
        return (bits[code >> 6] >> (code & 63)) & 1ull;
    }
};

// the present bits themselves
struct Always {
    using T = uint32_t;
    static constexpr bool kLoads = false;
    __device__ void init() {}
    __device__ bool operator()(uint32_t) const { return true; }
};

// a text column's row against a constant of up to 256 bytes (column_str.h has the predicate): the value is the row's
// 8-byte reference into the part's heap, which each lane reads for its own row with aligned dword loads; the constant is
// staged in LDS, one dword per thread.  A row at a position >= n_rows arrives as the reference 0: length 0, nothing read.
struct StrWhere {
    using T = uint64_t;   // {uint32 start, uint32 len}, little-endian
    static constexpr bool kLoads = true;
    struct Heap {
        const uint32_t *dwords;
        __device__ uint32_t operator()(uint32_t i) const { return dwords[i]; }
    };
    int op;
    Heap heap;
    const uint32_t *constant;  // device, ceil(len / 4) dwords
    uint32_t len;
    const uint32_t *lds;
    __device__ void init()
    {
        __shared__ uint32_t s[szgi::kStrPatternDwords];
        if (threadIdx.x < (len + 3) / 4) s[threadIdx.x] = constant[threadIdx.x];
        __syncthreads();
        lds = s;
    }
    __device__ bool operator()(uint64_t ref) const
    {
        return szgi::str_predicate(op, heap, (uint32_t)ref, (uint32_t)(ref >> 32), lds, len);
    }
};

// a text column's row through a byte automaton (column_dfa.h has the walk and the image): the block copies the class
// map -- and, kLdsTable, the staged table of at most kDfaLdsEntries entries -- into dynamic LDS, whose size the launch
// passes; a larger table is walked where it lies, in global memory, with plain cached loads.  Each lane then reads its
// own row's bytes with aligned dword loads until they end or an absorbing state is met; the accept bit of the state it
// ends in is one more global load.  The host has checked every entry of the tables: no index formed here leaves them.
template <bool kLdsTable>
struct DfaWhere {
    using T = uint64_t;   // {uint32 start, uint32 len}, little-endian
    static constexpr bool kLoads = true;
    StrWhere::Heap heap;
    const uint32_t *image;    // device: dfa_image_dwords() dwords
    const uint64_t *accept;   // device: ceil(n_states / 64) words
    uint32_t n_entries, n_classes, start;   // (start: staged)
    const uint8_t *class_of;
    const uint16_t *table;
    __device__ void init()
    {
        extern __shared__ uint32_t dfa_lds[];
        const uint32_t n = 64 + (kLdsTable ? (n_entries + 1) / 2 : 0);
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) dfa_lds[i] = image[i];
        __syncthreads();
        class_of = reinterpret_cast<const uint8_t *>(dfa_lds);
        table = reinterpret_cast<const uint16_t *>(kLdsTable ? dfa_lds + 64 : image + 64);
    }
    __device__ bool operator()(uint64_t ref) const
    {
        const uint8_t *cls = class_of;
        const uint16_t *tab = table;
        const uint32_t s = szgi::dfa_walk(
            heap, (uint32_t)ref, (uint32_t)(ref >> 32), [cls](uint32_t b) -> uint32_t { return cls[b]; },
            [tab](uint32_t i) -> uint32_t { return tab[i]; }, n_classes, start);
        return szgi::dfa_accepts(accept, s);
    }
};

// the bits of word w that stand for rows < n_rows
__device__ __forceinline__ uint64_t valid_bits(uint64_t w, uint64_t n_rows)
{
    const uint64_t lo = w * 64;
    if (lo >= n_rows) return 0ull;
    const uint64_t left = n_rows - lo;
    return left >= 64 ? ~0ull : ((1ull << left) - 1ull);
}

// out pair i = ballots of pred(values[row]) & present pair i (& base pair i), the tail cleared; the block's popcount
// goes to *count in one atomic add.  present null = every row present; base null = no base.
template <class Pred>
__global__ __launch_bounds__(256) void column_where_kernel(Pred pred, const typename Pred::T *__restrict__ values,
                                                           const ulonglong2 *__restrict__ present,
                                                           const ulonglong2 *__restrict__ base, ulonglong2 *__restrict__ out,
                                                           uint64_t n_pairs, uint64_t n_rows,
                                                           unsigned long long *__restrict__ count)
{
    using T = typename Pred::T;
    __shared__ unsigned int part[4];
    pred.init();
    const unsigned lane = threadIdx.x & 63;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    unsigned int ones = 0;  // (lane 0's is the wave's)
    for (uint64_t i0 = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i0 < n_pairs; i0 += n_waves * kSteps) {
        T v[kSteps][2];
#pragma unroll
        for (int s = 0; s < kSteps; s++) {
            const uint64_t r = (i0 + s * n_waves) * 128 + lane;   // (>= n_rows as well when the step is past n_pairs)
            v[s][0] = T(0), v[s][1] = T(0);
            if (Pred::kLoads) {
                if (r < n_rows) v[s][0] = values[r];
                if (r + 64 < n_rows) v[s][1] = values[r + 64];
            }
        }
#pragma unroll
        for (int s = 0; s < kSteps; s++) {
            const uint64_t i = i0 + s * n_waves;
            if (i >= n_pairs) break;   // (uniform over the wave)
            ulonglong2 w;
            w.x = __ballot(pred(v[s][0]));
            w.y = __ballot(pred(v[s][1]));
            if (lane == 0) {
                if (present) {
                    const ulonglong2 p = present[i];
                    w.x &= p.x, w.y &= p.y;
                }
                if (base) {
                    const ulonglong2 b = base[i];
                    w.x &= b.x, w.y &= b.y;
                }
                w.x &= valid_bits(2 * i, n_rows);
                w.y &= valid_bits(2 * i + 1, n_rows);
                out[i] = w;
                ones += (unsigned int)(__popcll(w.x) + __popcll(w.y));
            }
        }
    }
    if (lane == 0) part[threadIdx.x >> 6] = ones;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long sum = (unsigned long long)part[0] + part[1] + part[2] + part[3];
        if (sum) atomicAdd(count, sum);
    }
}

// lds: bytes of dynamic LDS the predicate's init() fills
template <class Pred>
hipError_t launch_where(const Pred &pred, const typename Pred::T *values, const ColumnWhere &w, hipStream_t stream,
                        size_t lds = 0)
{
    if (w.n_pairs == 0) return hipSuccess;
    if (w.n_rows > w.n_pairs * 128 || !w.out || !w.count) return hipErrorInvalidValue;
    const uint64_t blocks = (w.n_pairs + 4 * kSteps - 1) / (4 * kSteps);   // 4 waves x kSteps pairs per block and trip
    const unsigned grid = (unsigned)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks));
    hipLaunchKernelGGL(column_where_kernel<Pred>, dim3(grid), dim3(256), lds, stream, pred, values,
                       reinterpret_cast<const ulonglong2 *>(w.present), reinterpret_cast<const ulonglong2 *>(w.base),
                       reinterpret_cast<ulonglong2 *>(w.out), w.n_pairs, w.n_rows,
                       reinterpret_cast<unsigned long long *>(w.count));
    return hipGetLastError();
}

}  // namespace

hipError_t launch_column_cmp_f64(const double *values, int op, double constant, const ColumnWhere &w, hipStream_t stream)
{
    if (op < 0 || op > 5 || (!values && w.n_pairs)) return hipErrorInvalidValue;
    return launch_where(CmpF64{op, constant}, values, w, stream);
}

hipError_t launch_column_in_f64(const double *values, const double *sorted, uint32_t n_sorted, const ColumnWhere &w,
                                hipStream_t stream)
{
    if (n_sorted > (uint32_t)kColumnInMax || (!sorted && n_sorted) || (!values && w.n_pairs)) return hipErrorInvalidValue;
    return launch_where(InF64{sorted, n_sorted, nullptr}, values, w, stream);
}

hipError_t launch_column_codes_u32(const uint32_t *values, const uint64_t *code_bits, uint32_t n_codes, const ColumnWhere &w,
                                   hipStream_t stream)
{
    if ((!code_bits && n_codes) || (!values && w.n_pairs)) return hipErrorInvalidValue;
    return launch_where(CodeBits{code_bits, n_codes}, values, w, stream);
}

hipError_t launch_column_str(const uint64_t *refs, const uint8_t *heap, int op, const uint32_t *constant, uint32_t len,
                             const ColumnWhere &w, hipStream_t stream)
{
    static_assert(szgi::kStrPatternDwords <= 256, "StrWhere::init stages one dword per thread of the block");
    if (op < 0 || op > szgi::kStrOpContains || len > szgi::kStrPatternMax || (!constant && len) ||
        ((!refs || !heap) && w.n_pairs))
        return hipErrorInvalidValue;
    return launch_where(StrWhere{op, {reinterpret_cast<const uint32_t *>(heap)}, constant, len, nullptr}, refs, w, stream);
}

hipError_t launch_column_dfa(const uint64_t *refs, const uint8_t *heap, const uint32_t *image, const uint64_t *accept_bits,
                             uint32_t n_states, uint32_t n_classes, uint32_t start_staged, const ColumnWhere &w,
                             hipStream_t stream)
{
    const uint64_t n_entries = (uint64_t)n_states * n_classes;
    if (n_states == 0 || n_states > szgi::kDfaStatesMax || n_classes == 0 || n_classes > 256 || n_entries > szgi::kDfaTableMax ||
        (start_staged & (szgi::kDfaStop - 1)) >= n_states || !image || !accept_bits || ((!refs || !heap) && w.n_pairs))
        return hipErrorInvalidValue;
    const StrWhere::Heap h{reinterpret_cast<const uint32_t *>(heap)};
    if (n_entries <= szgi::kDfaLdsEntries)   // the class map and the table, an odd count of entries rounded up to a dword
        return launch_where(DfaWhere<true>{h, image, accept_bits, (uint32_t)n_entries, n_classes, start_staged, nullptr, nullptr},
                            refs, w, stream, 4 * szgi::dfa_image_dwords(n_states, n_classes));
    return launch_where(DfaWhere<false>{h, image, accept_bits, (uint32_t)n_entries, n_classes, start_staged, nullptr, nullptr},
                        refs, w, stream, 256);
}

hipError_t launch_column_present(const ColumnWhere &w, hipStream_t stream)
{
    return launch_where(Always{}, static_cast<const uint32_t *>(nullptr), w, stream);
}

}  // namespace szg
