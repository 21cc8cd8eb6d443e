// kernels_query_prep.hip -- a sketch batch's queries prepared on the card (option query_prep): from the float64 batch
// that is uploaded for the re-rank anyway to the 8-bit one-sweep image and the five constants of each query, by the rule
// of query_prep.h -- the bytes and the bit patterns the host form produces (prep_query, scan_query.cpp).  Compiled
// without contraction (-ffp-contract=off, like kernels_exact.hip); the two sums whose order matters are added by one
// lane, left to right, with explicit __dmul_rn / __dadd_rn.
//
// One workgroup per query.  Nothing here streams: a query is dim doubles (6 KiB at 768 dimensions), read from L2 three
// times, and the workgroup's time is the two chains of dim dependent float64 additions (m1, then qnorm2, which needs
// the scale that m1 gives).  256 threads: the products of a chunk of kChunk elements are written to LDS by all lanes, so
// that the adding lane finds them side by side, and the word build -- 3 r16 x 4 plane words, 576 at 768 dimensions, each
// with up to four divisions -- gets two to three words per lane; more threads would only lengthen the barriers the
// chain waits behind, fewer would put the word build's divisions (16 cycles of issue each at the float64 rate) in a
// row.  No atomics, no byte stores: a lane owns whole 32-bit plane words.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "query_prep.h"

namespace szg {

constexpr int kQpBlock = 256;
constexpr int kQpChunk = 1024;  // elements whose products lie in LDS at a time (8 KiB)

// the query's element e as the host's loop sees it: divided by the collection's scale where there is one
__device__ __forceinline__ double qp_elem(const double *q, int e, double gs) { return gs > 0.0 ? q[e] / gs : q[e]; }

// sum over e of (q_e * s)^2 in element order; every lane returns the sum
__device__ double qp_ordered_sum(const double *q, int dim, double gs, double s, double *prod, double *bcast)
{
    const int tid = threadIdx.x;
    double acc = 0.0;  // (lane 0's)
    for (int base = 0; base < dim; base += kQpChunk) {
        const int n = min(kQpChunk, dim - base);
        for (int i = tid; i < n; i += kQpBlock) {
            const double v = __dmul_rn(qp_elem(q, base + i, gs), s);
            prod[i] = __dmul_rn(v, v);
        }
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < n; i++) acc = __dadd_rn(acc, prod[i]);
        __syncthreads();
    }
    if (tid == 0) *bcast = acc;
    __syncthreads();
    const double r = *bcast;
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kQpBlock) void query_prep_kernel(const double *__restrict__ q64, int dim, double gs, int cosine,
                                                              int planes, int r16, uint32_t qsw_bytes,
                                                              uint8_t *__restrict__ qsw, double *__restrict__ meta)
{
    __shared__ double prod[kQpChunk];
    __shared__ double bcast;
    __shared__ double wmax[kQpBlock / 64];
    __shared__ long long wsum[kQpBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *q = q64 + (size_t)blockIdx.x * dim;

    // m1 = sum q^2 (q * 1.0 is q), the scale, qnorm2 = sum (q scale)^2
    const double m1 = qp_ordered_sum(q, dim, gs, 1.0, prod, &bcast);
    const double scale = qp_scale(cosine, 8, m1);
    const double qnorm2 = qp_ordered_sum(q, dim, gs, scale, prod, &bcast);

    // vmax: order-free under qp_max (a NaN never enters)
    double vmax = 0.0;
    for (int e = tid; e < dim; e += kQpBlock) vmax = qp_max(vmax, fabs(__dmul_rn(qp_elem(q, e, gs), scale)));
    for (int off = 32; off > 0; off >>= 1) vmax = qp_max(vmax, __shfl_down(vmax, off, 64));
    if (lane == 0) wmax[wave] = vmax;
    __syncthreads();
    vmax = wmax[0];
    for (int w = 1; w < kQpBlock / 64; w++) vmax = qp_max(vmax, wmax[w]);

    const double Qmax = qp_qmax8(planes);
    const double qs = qp_step(vmax, Qmax);

    // the plane words: word w of the image is plane w / (4 r16), piece (w / 4) % r16, dword w % 4 -- elements
    // 16 piece + 4 dword + 0 .. 3.  The planes below the top one stay zero, as do the bytes beyond dim.
    const int words = (int)(qsw_bytes / 4), per_plane = 4 * r16, top = 3 - planes;
    uint32_t *out = reinterpret_cast<uint32_t *>(qsw + (size_t)blockIdx.x * qsw_bytes);
    long long sumQ = 0;
    for (int w = tid; w < words; w += kQpBlock) {
        const int x = w / per_plane, e0 = (w - x * per_plane) * 4;
        uint32_t word = 0;
        if (x >= top && x <= 2) {
            for (int kb = 0; kb < 4; kb++) {
                const int e = e0 + kb;
                if (e >= dim) break;
                const long long Q = qp_quantize(qp_elem(q, e, gs), scale, qs, Qmax);
                if (x == 2) sumQ += Q;  // (every element has exactly one l-plane byte)
                word |= (uint32_t)((uint8_t)(int8_t)qp_digit(Q, x, planes)) << (8 * kb);
            }
        }
        out[w] = word;
    }
    for (int off = 32; off > 0; off >>= 1) sumQ += __shfl_down(sumQ, off, 64);
    if (lane == 0) wsum[wave] = sumQ;
    __syncthreads();
    if (tid == 0) {
        long long s = 0;
        for (int w = 0; w < kQpBlock / 64; w++) s += wsum[w];
        double *m = meta + (size_t)blockIdx.x * kQueryPrepMeta;
        m[kQpQnorm] = qp_canon(sqrt(qnorm2));
        m[kQpM1] = qp_canon(m1);
        m[kQpQscale] = qs;
        m[kQpQconst] = (double)s;
        m[kQpQnorm2] = qp_canon(qnorm2);
    }
}

hipError_t launch_query_prep(const double *d_q64, int nq, int dim, double gs, int cosine, int planes, int r16, uint32_t qsw_bytes,
                             uint8_t *d_qsw, double *d_meta, hipStream_t stream)
{
    if (nq < 1 || dim < 1 || (planes != 2 && planes != 3) || r16 < 1 || qsw_bytes != qp_image_bytes(r16) || dim > 16 * r16)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(query_prep_kernel, dim3((unsigned)nq), dim3(kQpBlock), 0, stream, d_q64, dim, gs, cosine, planes, r16,
                       qsw_bytes, d_qsw, d_meta);
    return hipGetLastError();
}

}  // namespace szg
