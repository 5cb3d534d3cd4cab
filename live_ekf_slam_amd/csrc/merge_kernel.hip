// merge_kernel.hip — merging duplicate landmarks of the EKF batch on the device (slam_map_duplicates, slam_merge_landmarks,
// slam_map_merge): the per-instance functions of merge_kernel.h mapped to gfx950.  ONE WORKGROUP PER INSTANCE, as map_compact_kernel.
//
// merge_find_kernel: the costs of all pairs and the mutual nearest neighbours.
//   mapping    a lane owns slot j = tid + k * 256 (one slot up to L_max = 256, else k < 4: L_max <= 1000 <= 4 * 256) and walks the other
//              slots t, so its running best (d2, slot) per owned slot stays in REGISTERS.  Each unordered pair is therefore costed twice,
//              once by either owner, through merge_pair_cost with the lower slot first: the same operands in the same order, hence the
//              same bits, and the cost is symmetric by construction.  Up to L_max = 64 one wavefront would own every slot and three
//              would idle: there all four own the slots j = lane and share the slots t among them (t mod 4), and wavefront 0 joins the
//              four bests of a slot through LDS with the same merge_consider (smallest d2, ties to the lowest slot: no order matters).
//   panels     for TP slots t at a time BOTH the rows tt, tt + 1 (the blocks (t, j), contiguous over the lanes j) and the columns
//              tt, tt + 1 (the transposed blocks (j, t), strided by two rows of P over the lanes: one line per lane and load if read
//              directly) are STAGED THROUGH LDS by the whole workgroup, lanes along row segments (whole rows for the row panel; 16 TP
//              bytes (fp64) of one line per row for the column panel, the neighbouring panels take the rest of the line from L2), with
//              kMergeStage = 8 loads in flight per lane.  The columns are stored TRANSPOSED, Ct[k][r], so that the lanes j read
//              Ct[k][jj + a] like the row panel, at a stride of two doubles (a two-way bank conflict of 8-byte reads, against the 64-way
//              one of the untransposed layout at a row stride of 16 doubles).  The diagonal block of t is a broadcast from the row panel.
//              TP is what 56 KiB of LDS hold, at most 8 (L_max = 1000: TP = 1, 64 KB).  The inner loop touches LDS and registers only.
//              All of P is thus read twice per find, both times in whole lines: once as row panels, once as column panels.  A first
//              version read the rows from global memory inside the loop over t and staged the columns with one load in flight per
//              lane, one wavefront per instance: 4.5 ms against 3.3 ms now at L = 50 x 65 536 fp64 (fp32: 4.3 and 4.4).
//   decision   nn [L_max] in LDS; ONE barrier between writing nn and the mutual test nn[nn[j]] == j.  An instance in which no slot has a
//              candidate leaves before it: it has written no output row (the launcher's caller presets them).
// merge_fuse_kernel: the sequential fusion of an instance's pairs IN PLACE in the canonical buffer, merge_fuse_instance over the 256
//   lanes, the workspace (4 n + 2 doubles, 64 KB at n = 2003) in dynamic LDS.  The gather of c_r is a column read (two lines per row and
//   pair, n rows) beside the n * ld elements the update streams through along rows; the two barriers per pair are argued in merge_kernel.h.
//   Index arithmetic inside an instance is int; b * pstride is formed in size_t.
// MergeWorkTerms: the traffic model, summed in integers by launch_work_sum outside any timed part.
// Record of the fusion: launch_record_reduce (record_kernel.h) with the join mask kMergeRecMax (entry kMrgMaxD2 is a maximum).
#include <hip/hip_runtime.h>

#include "../../include/slam_batch.h"
#include "aux_device.h"
#include "lds_attr.h"
#include "merge_kernel.h"

namespace slam {
namespace {

static_assert(kMergeRecLen == kRecLen, "the record launch_record_reduce takes");

constexpr int kMergeThreads = 256;                  // one instance's workgroup
constexpr int kMergeOwn = 4;                        // slots a lane of the find owns at most
constexpr int kMergePanelBytes = 56 * 1024;         // LDS of the find's two panels, where one slot of each fits into it
constexpr int kMergeStage = 8;                      // global loads a lane has in flight while a panel is staged
static_assert(kMergeOwn * kMergeThreads >= kMapMaxLandmarks, "every slot has an owner");

struct MergeGroup {
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int width() const { return kMergeThreads; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

// e-th element of a panel of `total` elements in kMergeStage rounds: all loads of a round are issued before its first LDS store, so a
// lane has kMergeStage global loads in flight (DESIGN.md 4.14 has the measurement beside one load per lane and round trip)
template <class ST, class Src, class Dst>
__device__ __forceinline__ void merge_stage(const ST* __restrict__ Pb, double* s, int total, int tid, int nth, Src src_of, Dst dst_of) {
    for (int e0 = 0; e0 < total; e0 += kMergeStage * nth) {
        double v[kMergeStage];
#pragma unroll
        for (int q = 0; q < kMergeStage; ++q) {
            const int e = e0 + q * nth + tid;
            v[q] = e < total ? (double)Pb[src_of(e)] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < kMergeStage; ++q) {
            const int e = e0 + q * nth + tid;
            if (e < total) s[dst_of(e)] = v[q];
        }
    }
}

// OWN: slots a lane owns (j = tid + k * width).  SPLIT (OWN = 1, L_max <= 64): the four wavefronts all own the slots j = lane and share
// the slots t of a panel among them (t mod 4), their four running bests joined through LDS by the same merge_consider at the end: every
// wavefront computes, where one alone would (the join is order-independent: smallest d2, ties to the lowest slot).
template <class ST, int OWN, bool SPLIT>
__global__ __launch_bounds__(kMergeThreads) void merge_find_kernel(const MergeFindParams p, const int TP, const int npad) {
    extern __shared__ double s_dyn[];                // the panel: [2 TP][npad] columns, transposed, then [2 TP][npad] rows
    __shared__ int s_nn[kMapMaxLandmarks];
    __shared__ double s_bd[SPLIT ? kMergeThreads : 1];
    __shared__ int s_bi[SPLIT ? kMergeThreads : 1];
    static_assert(!SPLIT || OWN == 1, "a split find owns one slot per lane");
    const int b = blockIdx.x;                        // (the grid is exactly B workgroups)
    const int tid = threadIdx.x, nth = blockDim.x;
    const int M = aux_clamp_m(p.M[b], p.L_max);
    if ((p.status[b] & kMapStatusSkip) || M < 2) return;   // (the whole workgroup, before any barrier: no pairs, nothing written)
    const int n = 3 + 2 * M, ld = ekf_ld(n, (int)sizeof(ST));
    const ST* __restrict__ const Pb = aux_row<ST>(p.P, b, p.pstride);
    const ST* __restrict__ const xb = aux_row<ST>(p.x, b, p.xstride);
    double* const s_ct = s_dyn;
    double* const s_rw = s_dyn + 2 * TP * npad;
    const int wv = SPLIT ? tid / 64 : 0, own0 = SPLIT ? tid % 64 : tid;
    const bool owner = !SPLIT || wv == 0;            // the lanes that hold the final best of their slots
    double xj[OWN][2], Pjj[OWN][4], bd[OWN];
    int bi[OWN];
#pragma unroll
    for (int k = 0; k < OWN; ++k) {
        const int j = own0 + k * nth, jj = 3 + 2 * j;
        bd[k] = __builtin_nan(""); bi[k] = -1;
        if (j < M) {
            xj[k][0] = (double)xb[jj]; xj[k][1] = (double)xb[jj + 1];
            Pjj[k][0] = (double)Pb[jj * ld + jj]; Pjj[k][1] = (double)Pb[jj * ld + jj + 1];
            Pjj[k][2] = (double)Pb[(jj + 1) * ld + jj]; Pjj[k][3] = (double)Pb[(jj + 1) * ld + jj + 1];
        } else {
            xj[k][0] = xj[k][1] = 0.0; Pjj[k][0] = Pjj[k][1] = Pjj[k][2] = Pjj[k][3] = 0.0;
        }
    }
    for (int t0 = 0; t0 < M; t0 += TP) {             // (uniform trip count: M is the workgroup's)
        const int tp = M - t0 < TP ? M - t0 : TP, cols = 2 * tp, c0 = 3 + 2 * t0;
        __syncthreads();                             // the panel before this one has been read by every lane
        // columns c0 .. c0 + cols of every row, stored transposed (r < n <= npad, c0 + k < n) ...
        merge_stage(Pb, s_ct, n * cols, tid, nth, [&](int e) { const int r = e / cols; return r * ld + c0 + (e - r * cols); },
                    [&](int e) { const int r = e / cols; return (e - r * cols) * npad + r; });
        // ... and rows c0 .. c0 + cols as they lie
        merge_stage(Pb, s_rw, cols * n, tid, nth, [&](int e) { const int k = e / n; return (c0 + k) * ld + (e - k * n); },
                    [&](int e) { const int k = e / n; return k * npad + (e - k * n); });
        __syncthreads();
        for (int u = wv; u < tp; u += SPLIT ? 4 : 1) {
            const int t = t0 + u, tt = 3 + 2 * t;
            const double* const ca = s_ct + (2 * u) * npad;      // column tt of P
            const double* const cb = ca + npad;                  // column tt + 1
            const double* const ra = s_rw + (2 * u) * npad;      // row tt of P
            const double* const rb = ra + npad;                  // row tt + 1
            const double xt0 = (double)xb[tt], xt1 = (double)xb[tt + 1];
            const double Ptt[4] = {ra[tt], ra[tt + 1], rb[tt], rb[tt + 1]};
#pragma unroll
            for (int k = 0; k < OWN; ++k) {
                const int j = own0 + k * nth, jj = 3 + 2 * j;
                if (j >= M || j == t) continue;
                const double Rt[4] = {ra[jj], ra[jj + 1], rb[jj], rb[jj + 1]};                   // block (t, j)
                const double Cj[4] = {ca[jj], cb[jj], ca[jj + 1], cb[jj + 1]};                   // block (j, t)
                const double d2 = t < j ? merge_pair_cost(xt0, xt1, xj[k][0], xj[k][1], Ptt, Rt, Cj, Pjj[k], p.sigma2)
                                        : merge_pair_cost(xj[k][0], xj[k][1], xt0, xt1, Pjj[k], Cj, Rt, Ptt, p.sigma2);
                merge_consider(d2, t, p.gate, &bd[k], &bi[k]);
            }
        }
    }
    if (SPLIT) {                                     // the four wavefronts' bests of slot j = lane, joined by wavefront 0
        s_bd[tid] = bd[0]; s_bi[tid] = bi[0];
        __syncthreads();
        if (owner)
            for (int w = 1; w < 4; ++w)
                if (s_bi[w * 64 + own0] >= 0) merge_consider(s_bd[w * 64 + own0], s_bi[w * 64 + own0], p.gate, &bd[0], &bi[0]);
    }
    bool any = false;
#pragma unroll
    for (int k = 0; k < OWN; ++k) {
        const int j = own0 + k * nth;
        if (owner && j < M) { s_nn[j] = bi[k]; any = any || bi[k] >= 0; }
    }
    if (p.find_on && tid == 0) p.find_on[b] = 1;
    if (!__syncthreads_or(any)) return;              // (the barrier the mutual test needs; no candidate: no output row is written)
    const size_t row = (size_t)b * p.L_max;
    int lonely = 0;
#pragma unroll
    for (int k = 0; k < OWN; ++k) {
        const int j = own0 + k * nth;
        if (owner && j < M) {
            const bool mutual = bi[k] >= 0 && s_nn[bi[k]] == j;
            p.partner[row + j] = mutual ? bi[k] : -1;
            if (p.d2) p.d2[row + j] = bd[k];
            lonely += (bi[k] >= 0 && !mutual) ? 1 : 0;
        }
    }
    lonely = __syncthreads_count(lonely & 1) + 2 * __syncthreads_count(lonely & 2) + 4 * __syncthreads_count(lonely & 4);
    if (tid == 0) p.n_notmutual[b] = lonely;
}

template <class ST>
__global__ __launch_bounds__(kMergeThreads) void merge_fuse_kernel(const MergeFuseParams p) {
    extern __shared__ double s_ws[];                 // 4 n + 2 doubles
    __shared__ uint16_t s_pi[kMapMaxLandmarks / 2], s_pj[kMapMaxLandmarks / 2];
    __shared__ int s_np, s_ig;
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int M = aux_clamp_m(p.M[b], p.L_max);
    const bool skip = (p.status[b] & kMapStatusSkip) != 0;
    const size_t row = (size_t)b * p.L_max;
    const int32_t* const partner = p.partner + row;
    if (tid < 64) {                                  // the honoured pairs in ascending i, and the entries that are not
        int np = 0, ig = 0;
        for (int s0 = 0; s0 < p.L_max; s0 += 64) {
            const int s = s0 + tid;
            const int32_t e = s < p.L_max ? partner[s] : -1;
            const bool hon = !skip && s < p.L_max && merge_honoured(partner, s, M);
            const bool first = hon && e > s;
            const unsigned long long mask = __ballot(first);
            if (first) {
                const int at = np + __popcll(mask & ((1ull << tid) - 1ull));
                s_pi[at] = (uint16_t)s; s_pj[at] = (uint16_t)e;
            }
            np += __popcll(mask);
            ig += __popcll(__ballot(!hon && e != -1));
        }
        if (tid == 0) { s_np = np; s_ig = ig; }
    }
    for (int s = tid; s < p.L_max; s += kMergeThreads) p.remove[row + s] = 0;
    __syncthreads();                                 // the pair list and the zeroed mask row
    const int np = s_np;
    MergeCounts cnt = {0, 0, 0.0, 0.0};
    if (np > 0) {
        cnt = merge_fuse_instance(MergeGroup(), aux_row<ST>(p.P, b, p.pstride), aux_row<ST>(p.x, b, p.xstride), M, s_pi, s_pj, np, p.sigma2, s_ws, p.remove + row, p.seen ? p.seen + row : nullptr,
                                  p.expected ? p.expected + row : nullptr);
    }
    if (tid == 0) {
        const int n = 3 + 2 * M;
        p.n_fused[b] = cnt.fused; p.n_attempted[b] = np;
        if (p.rec) {
            double* const r = p.inst_rec + (size_t)b * kMergeRecLen;
            for (int i = 0; i < kMergeRecLen; ++i) r[i] = 0.0;
            r[kMrgTouched] = cnt.fused > 0 ? 1.0 : 0.0;
            r[kMrgFused] = (double)cnt.fused;
            r[kMrgNotMutual] = (double)(s_ig + (p.n_notmutual ? p.n_notmutual[b] : 0));
            r[kMrgSingular] = (double)cnt.singular;
            r[kMrgUpdated] = (double)cnt.fused * ((double)n * (double)n);
            r[kMrgSumD2] = cnt.sum_d2; r[kMrgMaxD2] = cnt.max_d2;
        }
    }
}

// element i of the traffic model's sum: one instance of one call
struct MergeWorkTerms {
    const int32_t *M, *find_on, *n_attempted, *n_fused;
    int L_max, counters;
    __device__ void operator()(size_t i, unsigned long long (&t)[2]) const {
        const MergeTraffic w = merge_traffic(aux_clamp_m(M[i], L_max), find_on ? find_on[i] : 0, n_attempted[i], n_fused[i], L_max, counters != 0);
        t[0] = w.elems; t[1] = w.other_bytes;
    }
};

// the shape of a handle the find and the fusion take
bool merge_shape_ok(int B, int L_max, int pstride, int xstride, int f32_storage) {
    return aux_shape_ok(B, L_max, xstride, pstride, f32_storage) && L_max > 0 && L_max <= kMapMaxLandmarks;
}

}  // namespace

hipError_t launch_merge_find(const MergeFindParams& p, int f32_storage, hipStream_t stream) {
    if (!merge_shape_ok(p.B, p.L_max, p.pstride, p.xstride, f32_storage) || !p.P || !p.x || !p.M || !p.status || !p.partner || !p.n_notmutual)
        return hipErrorInvalidValue;
    const int npad = (3 + 2 * p.L_max) | 1;          // odd: the transposing stores of a row segment spread over the banks
    int TP = kMergePanelBytes / (32 * npad);
    TP = TP < 1 ? 1 : (TP > 8 ? 8 : TP);
    const size_t lds = sizeof(double) * 4 * (size_t)TP * npad;   // (<= 56 KiB, but 64 KB at L_max = 1000, where TP = 1)
    const int kind = p.L_max <= 64 ? 0 : (p.L_max <= kMergeThreads ? 1 : 2);   // split / one slot per lane / kMergeOwn slots per lane
    const void* const fns[2][3] = {
        {reinterpret_cast<const void*>(&merge_find_kernel<double, 1, true>), reinterpret_cast<const void*>(&merge_find_kernel<double, 1, false>),
         reinterpret_cast<const void*>(&merge_find_kernel<double, kMergeOwn, false>)},
        {reinterpret_cast<const void*>(&merge_find_kernel<float, 1, true>), reinterpret_cast<const void*>(&merge_find_kernel<float, 1, false>),
         reinterpret_cast<const void*>(&merge_find_kernel<float, kMergeOwn, false>)}};
    if (lds + 8192 > 64 * 1024) {   // once per device, to the kernel's maximum (lds_attr.h)
        const hipError_t e = slam_allow_full_lds(fns[f32_storage ? 1 : 0][kind]);
        if (e != hipSuccess) return e;
    }
    (void)hipGetLastError();   // sticky and per thread: only these launches' errors are reported (capi_internal.h)
    const dim3 grid(p.B), block(kMergeThreads);
    if (f32_storage) {
        if (kind == 0) hipLaunchKernelGGL((merge_find_kernel<float, 1, true>), grid, block, lds, stream, p, TP, npad);
        else if (kind == 1) hipLaunchKernelGGL((merge_find_kernel<float, 1, false>), grid, block, lds, stream, p, TP, npad);
        else hipLaunchKernelGGL((merge_find_kernel<float, kMergeOwn, false>), grid, block, lds, stream, p, TP, npad);
    } else {
        if (kind == 0) hipLaunchKernelGGL((merge_find_kernel<double, 1, true>), grid, block, lds, stream, p, TP, npad);
        else if (kind == 1) hipLaunchKernelGGL((merge_find_kernel<double, 1, false>), grid, block, lds, stream, p, TP, npad);
        else hipLaunchKernelGGL((merge_find_kernel<double, kMergeOwn, false>), grid, block, lds, stream, p, TP, npad);
    }
    return hipGetLastError();
}

hipError_t launch_merge_fuse(const MergeFuseParams& p, int f32_storage, hipStream_t stream) {
    if (!merge_shape_ok(p.B, p.L_max, p.pstride, p.xstride, f32_storage) || !p.P || !p.x || !p.M || !p.status || !p.partner || !p.remove ||
        !p.n_fused || !p.n_attempted || (p.rec && (!p.inst_rec || !p.partials)) || (p.seen == nullptr) != (p.expected == nullptr))
        return hipErrorInvalidValue;
    const size_t lds = sizeof(double) * (4 * (size_t)(3 + 2 * p.L_max) + 2);
    const void* fn = f32_storage ? reinterpret_cast<const void*>(&merge_fuse_kernel<float>) : reinterpret_cast<const void*>(&merge_fuse_kernel<double>);
    if (lds + 4096 > 64 * 1024) {   // once per device, to the kernel's maximum (lds_attr.h)
        const hipError_t e = slam_allow_full_lds(fn);
        if (e != hipSuccess) return e;
    }
    const hipError_t e = aux_launch(f32_storage, merge_fuse_kernel<float>, merge_fuse_kernel<double>, dim3(p.B), dim3(kMergeThreads), lds, stream, p);
    if (e != hipSuccess || !p.rec) return e;
    return launch_record_reduce<kMergeRecMax>(p.inst_rec, p.B, p.partials, p.rec, stream);
}

hipError_t launch_merge_work(const int32_t* M, const int32_t* find_on, const int32_t* n_attempted, const int32_t* n_fused, size_t n, int L_max,
                             int counters, unsigned long long* work, hipStream_t stream) {
    if (!M || !n_attempted || !n_fused) return hipErrorInvalidValue;
    return launch_work_sum<2>(MergeWorkTerms{M, find_on, n_attempted, n_fused, L_max, counters}, n, work, stream);
}

}  // namespace slam
