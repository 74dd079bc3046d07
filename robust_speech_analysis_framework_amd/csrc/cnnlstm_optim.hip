// The rest of the CNN-LSTM training step on gfx950, after the model's forward and backward (cnnlstm_train.hip): blob
// packing, cross-entropy, Adam, the gradient norm, BatchNorm running statistics; one launch per group each.  All of them
// are elementwise work on at most a few hundred thousand floats per replica.  The item descriptors travel by value in
// the kernel arguments, as the group recurrence kernels take theirs.
#include <cmath>

#include "cnnlstm_host.h"

namespace rsaf {
namespace cnntrain {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// the fixed tree of every sum of this file: 256 doubles of LDS, the total returned to every thread.  A second call on the
// same `part` needs a barrier in front of it (a thread may still be reading part[0]).
__device__ __forceinline__ double block_sum_256(double x, double* part) {
    part[threadIdx.x] = x;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    return part[0];
}

// One workgroup per item.  Rows are few (a batch) and classes fewer, so every row is computed in double by one lane
// and the row losses are summed by a fixed tree: the float results are the correctly rounded ones, deterministic.
struct CeItem {
    const float* logits;
    const long long* labels;
    float* loss;
    float* dlogits;
    const float* w;                             // class weights, or NULL: the unweighted mean
    int B;
};
struct CeGroup {
    CeItem item[RSAF_CNNLSTM_GROUP_MAX];
};

// the sum of the exponentials of a row of logits with its maximum subtracted, and that maximum
__device__ __forceinline__ double ce_row(const float* row, int nc, float* max_out) {
    float mx = row[0];
    for (int c = 1; c < nc; ++c) mx = fmaxf(mx, row[c]);
    double s = 0.0;
    for (int c = 0; c < nc; ++c) s += exp((double)row[c] - (double)mx);
    *max_out = mx;
    return s;
}

__device__ __forceinline__ void ce_item_mean(const CeItem& it, int nc, double* part) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < it.B; b += 256) {
        const float* row = it.logits + (int64_t)b * nc;
        float mx;
        const double s = ce_row(row, nc, &mx);
        const long long lab = it.labels[b];
        const bool ok = lab >= 0 && lab < nc;
        const double lse = (double)mx + log(s);
        acc += ok ? lse - (double)row[ok ? lab : 0] : __builtin_nan("");
        if (it.dlogits) {
            const double inv = 1.0 / (s * it.B);
            for (int c = 0; c < nc; ++c) {
                const double p = exp((double)row[c] - (double)mx) * inv;
                it.dlogits[(int64_t)b * nc + c] = (float)(ok && c == lab ? p - 1.0 / it.B : p);
            }
        }
    }
    const double total = block_sum_256(acc, part);
    if (threadIdx.x == 0) it.loss[0] = (float)(total / it.B);
}

// nn.CrossEntropyLoss(weight = w): loss = sum_b w[y_b] nll_b / sum_b w[y_b], dlogits_b = w[y_b] (softmax - onehot) / sum_b w[y_b].
// Both sums go through the tree of ce_item_mean; the gradient needs the second one, so the rows are walked twice (a batch
// of rows of at most 16 classes: the exponentials are cheaper than a round trip through memory).  An item without weights
// runs ce_item_mean itself: that is rsaf_ce_loss_group, whose every item comes without weights.
__global__ __launch_bounds__(256) void ce_loss_weighted_group_kernel(const CeGroup g, int nc) {
    const CeItem& it = g.item[blockIdx.x];
    __shared__ double part[256];
    if (!it.w) {
        ce_item_mean(it, nc, part);
        return;
    }
    double acc = 0.0, accw = 0.0;
    for (int b = threadIdx.x; b < it.B; b += 256) {
        const float* row = it.logits + (int64_t)b * nc;
        float mx;
        const double s = ce_row(row, nc, &mx);
        const long long lab = it.labels[b];
        const bool ok = lab >= 0 && lab < nc;
        const double lse = (double)mx + log(s);
        const double wb = ok ? (double)it.w[lab] : __builtin_nan("");
        acc += wb * (lse - (double)row[ok ? lab : 0]);
        accw += wb;
    }
    const double num = block_sum_256(acc, part);
    __syncthreads();                            // every thread has read part[0] before the next sum writes it
    const double wsum = block_sum_256(accw, part);
    if (threadIdx.x == 0) it.loss[0] = (float)(num / wsum);
    if (!it.dlogits) return;
    for (int b = threadIdx.x; b < it.B; b += 256) {
        const float* row = it.logits + (int64_t)b * nc;
        float mx;
        const double s = ce_row(row, nc, &mx);
        const long long lab = it.labels[b];
        const bool ok = lab >= 0 && lab < nc;
        const double wb = ok ? (double)it.w[lab] : __builtin_nan("");
        for (int c = 0; c < nc; ++c) {
            const double p = exp((double)row[c] - (double)mx) / s;
            it.dlogits[(int64_t)b * nc + c] = (float)(wb * (c == lab ? p - 1.0 : p) / wsum);
        }
    }
}

// Adam and the packing of the parameter blob.  A segment is one parameter tensor (ADAM_PLAIN, ADAM_CONV) or the
// b_ih / b_hh pair of one direction (ADAM_BIAS) and maps to a run of the blob.  Threads walk the PARAMETER's index space
// four floats at a time, so the parameter-side streams (p, m, v read and written) are full-width vector accesses; the
// blob side (gradient read in adam_group_kernel, blob write in pack_group_kernel) is contiguous too except for conv
// kernels, whose blob image is tap-major: there a wave's 256 consecutive [Cin][k] elements fall into k contiguous runs
// of the blob, which it gathers or scatters by dword.
enum { ADAM_PLAIN = 0, ADAM_CONV = 1, ADAM_BIAS = 2 };
static const int ADAM_MAX_SEGS = 56;            // 5 * 4 + 4 layers * 6 + 4 = 48 at most
static const int ADAM_BLOCK_FLOATS = 1024;      // 256 threads x 4

struct AdamSeg {
    int blob_off, n, block0;                    // first blob float | floats | first workgroup of the segment
    int cin;                                    // ADAM_CONV: the kernel is [Cout][cin][taps] in torch, [Cout][taps][cin] in the blob
    unsigned char kind, taps, pa, pb;           // parameter numbers (pb: ADAM_BIAS only)
};
struct AdamRep {
    const float* grads;                         // gradient blob or NULL (gradients by the table's fourth row)
    const unsigned long long* table;            // [3 or 4][P] device pointers
    unsigned long long skip;
    double step_size, b1, b2, eps, inv_sqrt_bc2;
};
// the segments of one architecture, as every kernel that walks them takes them; P: the number of parameters
struct SegTable {
    AdamSeg seg[ADAM_MAX_SEGS];
    int nseg, P;
};

// the segment of this workgroup; q0: the first of this thread's four elements in it (the parameter's index space)
__device__ __forceinline__ AdamSeg find_segment(const SegTable& T, int* q0) {
    int s = 0;
    while (s + 1 < T.nseg && (int)blockIdx.x >= T.seg[s + 1].block0) ++s;
    *q0 = (((int)blockIdx.x - T.seg[s].block0) * 256 + (int)threadIdx.x) * 4;
    return T.seg[s];
}

struct AdamGroup {
    SegTable t;
    AdamRep rep[RSAF_CNNLSTM_GROUP_MAX];
};
static_assert(sizeof(AdamGroup) <= 3584, "the descriptors must fit the kernel argument segment");

// SCALED: the gradient is g * scale (clipping by the norm, grad_norm_* below), the product rounded once in double; a
// scale of exactly 1 leaves g, so the update is the unscaled one bit for bit.
template <bool SCALED>
__device__ __forceinline__ float adam_one(float p, float g, float& m, float& v, const AdamRep& r, double scale) {
    const double gd = SCALED ? __dmul_rn((double)g, scale) : (double)g;
    const double md = r.b1 * (double)m + (1.0 - r.b1) * gd;
    const double vd = r.b2 * (double)v + (1.0 - r.b2) * gd * gd;
    m = (float)md;
    v = (float)vd;
    return (float)((double)p - r.step_size * md / (sqrt(vd) * r.inv_sqrt_bc2 + r.eps));
}

struct AdamTensor {
    float *p, *m, *v;
    const float* g;                             // gradient in the parameter's layout, or NULL
};

__device__ __forceinline__ AdamTensor adam_tensor(const AdamGroup& G, const AdamRep& r, int idx) {
    AdamTensor t;
    t.p = reinterpret_cast<float*>(r.table[idx]);
    t.m = reinterpret_cast<float*>(r.table[G.t.P + idx]);
    t.v = reinterpret_cast<float*>(r.table[2 * G.t.P + idx]);
    t.g = r.grads ? nullptr : reinterpret_cast<const float*>(r.table[3 * G.t.P + idx]);
    return t;
}

__device__ __forceinline__ bool aligned16(const AdamTensor& t) {
    return ((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.m) | reinterpret_cast<uintptr_t>(t.v) |
             reinterpret_cast<uintptr_t>(t.g)) & 15) == 0;
}

// blob index (relative to the segment) of element q of a conv kernel [Cout][cin][taps]
__device__ __forceinline__ int conv_blob_index(int q, int cin, int taps) {
    const int tap = q % taps, r = q / taps;
    const int co = r / cin, ci = r - co * cin;
    return (co * taps + tap) * cin + ci;
}

template <bool SCALED>
__device__ __forceinline__ void adam_group_body(const AdamGroup& G, double scale) {
    const AdamRep& r = G.rep[blockIdx.y];
    int q0;
    const AdamSeg sg = find_segment(G.t, &q0);
    const bool skip_a = (r.skip >> sg.pa) & 1, skip_b = sg.kind != ADAM_BIAS || ((r.skip >> sg.pb) & 1);
    if (skip_a && skip_b) return;
    if (q0 >= sg.n) return;
    const float* gblob = r.grads ? r.grads + sg.blob_off : nullptr;

    if (sg.kind == ADAM_BIAS) {                 // the blob holds b_ih + b_hh: both receive the gradient of the sum
        const AdamTensor a = adam_tensor(G, r, sg.pa), b = adam_tensor(G, r, sg.pb);
        for (int q = q0; q < min(q0 + 4, sg.n); ++q) {
            if (!skip_a) {
                float m = a.m[q], v = a.v[q];
                a.p[q] = adam_one<SCALED>(a.p[q], gblob ? gblob[q] : a.g[q], m, v, r, scale);
                a.m[q] = m; a.v[q] = v;
            }
            if (!skip_b) {
                float m = b.m[q], v = b.v[q];
                b.p[q] = adam_one<SCALED>(b.p[q], gblob ? gblob[q] : b.g[q], m, v, r, scale);
                b.m[q] = m; b.v[q] = v;
            }
        }
        return;
    }

    const AdamTensor t = adam_tensor(G, r, sg.pa);
    const bool conv = sg.kind == ADAM_CONV;
    if (q0 + 4 <= sg.n && aligned16(t)) {
        f32x4 p = *reinterpret_cast<const f32x4*>(t.p + q0);
        f32x4 m = *reinterpret_cast<const f32x4*>(t.m + q0);
        f32x4 v = *reinterpret_cast<const f32x4*>(t.v + q0);
        f32x4 g;
        if (t.g) g = *reinterpret_cast<const f32x4*>(t.g + q0);
        else if (!conv) g = *reinterpret_cast<const f32x4*>(gblob + q0);
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = gblob[conv_blob_index(q0 + j, sg.cin, sg.taps)];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {           // constant indices after unrolling: the vectors stay in registers
            float mj = m[j], vj = v[j];
            p[j] = adam_one<SCALED>(p[j], g[j], mj, vj, r, scale);
            m[j] = mj; v[j] = vj;
        }
        *reinterpret_cast<f32x4*>(t.p + q0) = p;
        *reinterpret_cast<f32x4*>(t.m + q0) = m;
        *reinterpret_cast<f32x4*>(t.v + q0) = v;
        return;
    }
    for (int q = q0; q < min(q0 + 4, sg.n); ++q) {            // tail of a segment, or tensors off the 16-byte grid
        const int bi = conv ? conv_blob_index(q, sg.cin, sg.taps) : q;
        float m = t.m[q], v = t.v[q];
        t.p[q] = adam_one<SCALED>(t.p[q], t.g ? t.g[q] : gblob[bi], m, v, r, scale);
        t.m[q] = m; t.v[q] = v;
    }
}

__global__ __launch_bounds__(256) void adam_group_kernel(const AdamGroup G) { adam_group_body<false>(G, 1.0); }

// one device float per replica (NULL: 1), read by every thread of the replica's workgroups
struct AdamScales {
    const float* scale[RSAF_CNNLSTM_GROUP_MAX];
};

__global__ __launch_bounds__(256) void adam_scaled_group_kernel(const AdamGroup G, const AdamScales S) {
    const float* sp = S.scale[blockIdx.y];
    adam_group_body<true>(G, sp ? (double)sp[0] : 1.0);
}

// The 2-norm of a replica's gradient as clip_grad_norm_ takes it: over the PARAMETERS that the step updates.  The walk
// is adam_group_kernel's (same segments, same workgroups, the parameter's index space), so a conv kernel is read through
// the same permutation, the padding between segments is never read, and a bias segment of the blob counts once per live
// parameter of its pair.  Every workgroup sums the squares of its <= 1024 floats in double (a float squared is exact
// there) through a fixed tree and writes ONE partial; grad_norm_finish_kernel sums a replica's partials in a fixed order.
// No atomics: the result depends on the gradients alone, not on K, on the replica's place in the group or on scheduling.
struct NormRep {
    const float* grads;                         // gradient blob or NULL (gradients by the table's fourth row)
    const unsigned long long* table;            // [4][P] device pointers when grads is NULL (only the fourth row is read)
    unsigned long long skip;
    double max_norm;
    double* partials;                           // [blocks]
    float *norm_out, *scale_out;
};
struct NormGroup {
    SegTable t;
    NormRep rep[RSAF_CNNLSTM_GROUP_MAX];
    int blocks;
};
static_assert(sizeof(NormGroup) <= 3584, "the descriptors must fit the kernel argument segment");

__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const NormGroup G) {
    const NormRep& r = G.rep[blockIdx.y];
    __shared__ double part[256];
    int q0;
    const AdamSeg sg = find_segment(G.t, &q0);
    const bool bias = sg.kind == ADAM_BIAS;
    const bool live_a = !((r.skip >> sg.pa) & 1), live_b = bias && !((r.skip >> sg.pb) & 1);
    double acc = 0.0;
    if (live_a || live_b) {
        const float* gblob = r.grads ? r.grads + sg.blob_off : nullptr;
        const float* ga = gblob || !live_a ? nullptr : reinterpret_cast<const float*>(r.table[3 * G.t.P + sg.pa]);
        const float* gb = gblob || !live_b ? nullptr : reinterpret_cast<const float*>(r.table[3 * G.t.P + sg.pb]);
        const bool conv = sg.kind == ADAM_CONV;
        for (int q = q0; q < min(q0 + 4, sg.n); ++q) {
            const int bi = conv ? conv_blob_index(q, sg.cin, sg.taps) : q;
            if (live_a) {
                const double g = gblob ? gblob[bi] : ga[q];
                acc += g * g;
            }
            if (live_b) {
                const double g = gblob ? gblob[bi] : gb[q];
                acc += g * g;
            }
        }
    }
    const double total = block_sum_256(acc, part);
    if (threadIdx.x == 0) r.partials[blockIdx.x] = total;
}

// grid K: norm = sqrt(sum of the partials), scale = min(1, max_norm / (norm + 1e-6)), both rounded to float once
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const NormGroup G) {
    const NormRep& r = G.rep[blockIdx.x];
    __shared__ double part[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < G.blocks; i += 256) acc += r.partials[i];
    const double total = block_sum_256(acc, part);
    if (threadIdx.x == 0) {
        const double norm = sqrt(total), ratio = r.max_norm / (norm + 1e-6);
        r.norm_out[0] = (float)norm;
        r.scale_out[0] = (float)(ratio < 1.0 || ratio != ratio ? ratio : 1.0);      // a NaN norm gives a NaN scale, as torch's clamp does
    }
}

// The parameter blob of the next forward, read from the parameters where they live: one launch per group step instead of
// ~35 slice assignments per replica, and nothing resident that an edit of the parameters could leave stale.
struct PackRep {
    const unsigned long long* table;            // [>= 1][P] device pointers: row 0 = the parameters
    float* blob;
};
struct PackGroup {
    SegTable t;
    PackRep rep[RSAF_CNNLSTM_GROUP_MAX];
};
static_assert(sizeof(PackGroup) <= 3584, "the descriptors must fit the kernel argument segment");

__global__ __launch_bounds__(256) void pack_group_kernel(const PackGroup G) {
    const PackRep& r = G.rep[blockIdx.y];
    int q0;
    const AdamSeg sg = find_segment(G.t, &q0);
    if (q0 >= sg.n) return;
    float* blob = r.blob + sg.blob_off;
    const float* a = reinterpret_cast<const float*>(r.table[sg.pa]);
    const float* b = sg.kind == ADAM_BIAS ? reinterpret_cast<const float*>(r.table[sg.pb]) : nullptr;
    const bool conv = sg.kind == ADAM_CONV;
    if (q0 + 4 <= sg.n && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0) {
        f32x4 p = *reinterpret_cast<const f32x4*>(a + q0);
        if (b) p += *reinterpret_cast<const f32x4*>(b + q0);
        if (!conv) *reinterpret_cast<f32x4*>(blob + q0) = p;
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j) blob[conv_blob_index(q0 + j, sg.cin, sg.taps)] = p[j];
        }
        return;
    }
    for (int q = q0; q < min(q0 + 4, sg.n); ++q)
        blob[conv ? conv_blob_index(q, sg.cin, sg.taps) : q] = b ? a[q] + b[q] : a[q];
}

// the segments of one architecture, in the parameter numbering of rsaf_cnnlstm_adam_group (include/rsaf.h)
static int make_adam_segs(const Dims& d, AdamSeg* segs, int* nseg, int64_t* blocks) {
    const PLayout L = make_playout(d);
    int n = 0, P = 0;
    int64_t blk = 0;
    auto add = [&](int kind, int64_t off, int64_t floats, int taps, int cin, int pa, int pb) {
        AdamSeg& sg = segs[n++];
        sg.blob_off = (int)off; sg.n = (int)floats; sg.block0 = (int)blk;
        sg.cin = cin; sg.kind = (unsigned char)kind; sg.taps = (unsigned char)taps;
        sg.pa = (unsigned char)pa; sg.pb = (unsigned char)pb;
        blk += (floats + ADAM_BLOCK_FLOATS - 1) / ADAM_BLOCK_FLOATS;
    };
    auto conv = [&](const ConvP& c, int taps, int cin) {
        add(taps > 1 ? ADAM_CONV : ADAM_PLAIN, c.w, (int64_t)d.C * taps * cin, taps, cin, P, 0);
        add(ADAM_PLAIN, c.b, d.C, 1, 0, P + 1, 0);
        add(ADAM_PLAIN, c.g, d.C, 1, 0, P + 2, 0);
        add(ADAM_PLAIN, c.be, d.C, 1, 0, P + 3, 0);
        P += 4;
    };
    conv(L.c1, 3, d.D);
    if (d.D != d.C) conv(L.sc, 1, d.D);
    conv(L.c2, 3, d.C); conv(L.c3, 3, d.C); conv(L.c4, 3, d.C);
    for (int l = 0; l < d.L; ++l) {
        const int64_t in = l == 0 ? d.C : 2 * d.H, nih = (int64_t)4 * d.H * in, nhh = (int64_t)4 * d.H * d.H;
        add(ADAM_PLAIN, L.wih[l], nih, 1, 0, P, 0);
        add(ADAM_PLAIN, L.wih[l] + nih, nih, 1, 0, P + 1, 0);
        add(ADAM_BIAS, L.bsum[l], 4 * d.H, 1, 0, P + 2, P + 3);
        add(ADAM_BIAS, L.bsum[l] + 4 * d.H, 4 * d.H, 1, 0, P + 4, P + 5);
        add(ADAM_PLAIN, L.whh[l], nhh, 1, 0, P + 6, 0);
        add(ADAM_PLAIN, L.whh[l] + nhh, nhh, 1, 0, P + 7, 0);
        P += 8;
    }
    add(ADAM_PLAIN, L.watt, 2 * d.H, 1, 0, P, 0);
    add(ADAM_PLAIN, L.batt, 1, 1, 0, P + 1, 0);
    add(ADAM_PLAIN, L.wfc, (int64_t)d.NC * 2 * d.H, 1, 0, P + 2, 0);
    add(ADAM_PLAIN, L.bfc, d.NC, 1, 0, P + 3, 0);
    P += 4;
    *nseg = n;
    *blocks = blk;
    return P;
}

// the byte ranges that the items of one call write; add() refuses a range that overlaps an earlier one, naming both
struct WriteRanges {
    struct Range { const char* p; int64_t bytes; int item; const char* what; };
    Range r[RSAF_CNNLSTM_GROUP_MAX * 3];
    int n = 0;
    int add(const void* p, int64_t bytes, int item, const char* what, const char* who) {
        if (!p) return RSAF_OK;
        const char* c = static_cast<const char*>(p);
        for (int i = 0; i < n; ++i)
            if (c < r[i].p + r[i].bytes && r[i].p < c + bytes)
                return fail(RSAF_ERR_ARG, who, item, (std::string("`") + what + "` overlaps `" + r[i].what + "` of item " +
                                                      std::to_string(r[i].item)).c_str());
        r[n++] = Range{c, bytes, item, what};
        return RSAF_OK;
    }
};

struct BnRunItem {
    const float* stats;
    float* mean[5];
    float* var[5];
    double momentum[5], unbias[5];
};
struct BnRunGroup {
    BnRunItem item[RSAF_CNNLSTM_GROUP_MAX];
};

// grid (C / 256, 5 layers, K)
__global__ __launch_bounds__(256) void bn_running_group_kernel(const BnRunGroup g, int C) {
    const BnRunItem& it = g.item[blockIdx.z];
    const int i = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C || !it.mean[i]) return;
    // running.mul_(1 - m).add_(batch, alpha = m [* n / (n - 1)]) with the scalars rounded to float as torch rounds them
    const float keep = (float)(1.0 - it.momentum[i]), am = (float)it.momentum[i], av = (float)(it.momentum[i] * it.unbias[i]);
    it.mean[i][c] = __fmaf_rn(am, it.stats[(i * 3 + 0) * C + c], __fmul_rn(it.mean[i][c], keep));
    it.var[i][c] = __fmaf_rn(av, it.stats[(i * 3 + 1) * C + c], __fmul_rn(it.var[i][c], keep));
}

// what RSAF_CHECK_HIP(hipGetLastError()) gives inside the entry `who`
static int launched(const char* who) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RSAF_OK : fail(RSAF_ERR_HIP, who, -1, (std::string("hipGetLastError() -> ") + hipGetErrorString(e)).c_str());
}

// What every entry over the segments opens with, in this order: the dims, K, items_host, the size of the blob, the
// segments.  `who`: the entry that was called.
static int seg_prepare(const Dims& d, const void* items_host, int K, const char* who, SegTable* T, int64_t* blocks, int64_t* total) {
    TRY(check_dims(d));
    TRY(check_group_args(K, items_host, who));
    *total = make_playout(d).total;
    if (!(*total <= 0x3fffffffLL && d.D <= 0xffffff)) return fail(RSAF_ERR_ARG, who, -1, "parameter blob too large");
    T->P = make_adam_segs(d, T->seg, &T->nseg, blocks);
    if (!(T->P <= 64 && *blocks <= 0x7fffffffLL)) return fail(RSAF_ERR_ARG, who, -1, "too many parameters");
    return RSAF_OK;
}

// both cross-entropy entries; WEIGHTED: ItemT carries class_weight, and items whose outputs overlap are refused (the
// unweighted entry goes on accepting them)
template <bool WEIGHTED, typename ItemT>
static int ce_loss_group(const ItemT* items_host, int K, int num_classes, hipStream_t s, const char* who) {
    TRY(check_group_args(K, items_host, who));
    if (!(num_classes >= 2)) return fail(RSAF_ERR_ARG, who, -1, "num_classes must be >= 2");
    CeGroup g{};
    WriteRanges writes;
    double bytes = 0.0;
    for (int k = 0; k < K; ++k) {
        const ItemT& it = items_host[k];
        if (!(it.B >= 1 && (int64_t)it.B * num_classes <= 0x3fffffffLL)) return fail(RSAF_ERR_ARG, who, k, "batch must be >= 1 and B * num_classes < 2^30");
        if (!(it.logits && it.labels && it.loss_out)) return fail(RSAF_ERR_ARG, who, k, "NULL pointer");
        if (WEIGHTED) TRY(writes.add(it.loss_out, 4, k, "loss_out", who));
        if (WEIGHTED) TRY(writes.add(it.dlogits_out, (int64_t)it.B * num_classes * 4, k, "dlogits_out", who));
        const float* w = nullptr;
        if constexpr (WEIGHTED) w = it.class_weight;
        g.item[k] = CeItem{it.logits, reinterpret_cast<const long long*>(it.labels), it.loss_out, it.dlogits_out, w, it.B};
        bytes += (double)it.B * (num_classes * (it.dlogits_out ? 8 : 4) + 8) + (w ? num_classes * 4.0 : 0.0);
    }
    ProfScope prof("train_ce", s, 0.0, bytes);
    hipLaunchKernelGGL(ce_loss_weighted_group_kernel, dim3(K), dim3(256), 0, s, g, num_classes);
    return launched(who);
}

// both Adam entries: the checks, the descriptors and the launch; SCALED: ItemT carries grad_scale
template <bool SCALED, typename ItemT>
static int adam_group(const Dims& d, const ItemT* items_host, int K, hipStream_t s, const char* who) {
    AdamGroup G{};
    AdamScales S{};
    int64_t blocks = 0, total = 0;
    TRY(seg_prepare(d, items_host, K, who, &G.t, &blocks, &total));
    for (int k = 0; k < K; ++k) {
        const ItemT& it = items_host[k];
        if (!it.table) return fail(RSAF_ERR_ARG, who, k, "NULL pointer");
        if (reinterpret_cast<uintptr_t>(it.grads) & 15) return fail(RSAF_ERR_ARG, who, k, "grads must be 16-byte aligned");
        if (!(it.step >= 1)) return fail(RSAF_ERR_ARG, who, k, "step counts from 1");
        if (!(it.beta1 >= 0.0 && it.beta1 < 1.0 && it.beta2 >= 0.0 && it.beta2 < 1.0 && it.eps >= 0.0 && it.lr >= 0.0))
            return fail(RSAF_ERR_ARG, who, k, "needs 0 <= beta < 1, eps >= 0, lr >= 0");
        for (int j = 0; j < k; ++j)
            if (items_host[j].table == it.table)
                return fail(RSAF_ERR_ARG, who, k, ("shares its table with item " + std::to_string(j)).c_str());
        AdamRep& r = G.rep[k];
        r.grads = it.grads;
        r.table = reinterpret_cast<const unsigned long long*>(it.table);
        r.skip = it.skip;
        r.b1 = it.beta1; r.b2 = it.beta2; r.eps = it.eps;
        r.step_size = it.lr / (1.0 - std::pow(it.beta1, (double)it.step));
        r.inv_sqrt_bc2 = 1.0 / std::sqrt(1.0 - std::pow(it.beta2, (double)it.step));
        if constexpr (SCALED) S.scale[k] = it.grad_scale;
    }
    ProfScope prof("train_adam", s, 0.0, (double)K * total * 4 * 7);
    if (SCALED) hipLaunchKernelGGL(adam_scaled_group_kernel, dim3((unsigned)blocks, K), dim3(256), 0, s, G, S);
    else hipLaunchKernelGGL(adam_group_kernel, dim3((unsigned)blocks, K), dim3(256), 0, s, G);
    return launched(who);
}

}  // namespace cnntrain
}  // namespace rsaf

using namespace rsaf;
using namespace rsaf::cnntrain;

extern "C" {

int rsaf_ce_loss_group(const rsaf_ce_loss_item* items_host, int K, int num_classes, rsaf_stream_t stream) {
    return ce_loss_group<false>(items_host, K, num_classes, (hipStream_t)stream, __func__);
}

int rsaf_ce_loss_weighted_group(const rsaf_ce_loss_weighted_item* items_host, int K, int num_classes, rsaf_stream_t stream) {
    return ce_loss_group<true>(items_host, K, num_classes, (hipStream_t)stream, __func__);
}

int rsaf_cnnlstm_adam_param_count(int input_dim, int channels, int hidden, int num_classes, int lstm_layers) {
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, ACT_SILU};
    if (check_dims(d) != RSAF_OK) return -1;
    return (d.D != d.C ? 20 : 16) + 8 * d.L + 4;
}

int rsaf_cnnlstm_adam_group(const rsaf_cnnlstm_adam_item* items_host, int K, int input_dim, int channels, int hidden,
                            int num_classes, int lstm_layers, rsaf_stream_t stream) {
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, ACT_SILU};
    return adam_group<false>(d, items_host, K, (hipStream_t)stream, __func__);
}

int rsaf_cnnlstm_adam_scaled_group(const rsaf_cnnlstm_adam_scaled_item* items_host, int K, int input_dim, int channels, int hidden,
                                   int num_classes, int lstm_layers, rsaf_stream_t stream) {
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, ACT_SILU};
    return adam_group<true>(d, items_host, K, (hipStream_t)stream, __func__);
}

int64_t rsaf_cnnlstm_grad_norm_partials(int input_dim, int channels, int hidden, int num_classes, int lstm_layers) {
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, ACT_SILU};
    if (check_dims(d) != RSAF_OK) return -1;
    SegTable T;                                 // no items and no launch here: the dims decide alone, as they always did
    int64_t blocks = 0;
    make_adam_segs(d, T.seg, &T.nseg, &blocks);
    return blocks;
}

int rsaf_cnnlstm_grad_norm_group(const rsaf_cnnlstm_grad_norm_item* items_host, int K, int input_dim, int channels, int hidden,
                                 int num_classes, int lstm_layers, rsaf_stream_t stream) {
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, ACT_SILU};
    NormGroup G{};
    int64_t blocks = 0, total = 0;
    TRY(seg_prepare(d, items_host, K, __func__, &G.t, &blocks, &total));
    G.blocks = (int)blocks;
    WriteRanges writes;
    for (int k = 0; k < K; ++k) {
        const rsaf_cnnlstm_grad_norm_item& it = items_host[k];
        if (!(it.grads || it.table)) return fail(RSAF_ERR_ARG, __func__, k, "NULL pointer: needs a gradient blob or a table with a fourth row");
        if (!(it.partials && it.norm_out && it.scale_out)) return fail(RSAF_ERR_ARG, __func__, k, "NULL pointer");
        if (reinterpret_cast<uintptr_t>(it.grads) & 15) return fail(RSAF_ERR_ARG, __func__, k, "grads must be 16-byte aligned");
        if (!(it.max_norm > 0.0)) return fail(RSAF_ERR_ARG, __func__, k, "max_norm must be > 0 and not NaN (+inf: no clipping)");
        if (reinterpret_cast<uintptr_t>(it.partials) & 7) return fail(RSAF_ERR_ARG, __func__, k, "partials must be 8-byte aligned");
        if (it.partials_count < blocks)
            return fail(RSAF_ERR_WORKSPACE, __func__, k, "partials is shorter than rsaf_cnnlstm_grad_norm_partials() doubles");
        TRY(writes.add(it.partials, blocks * 8, k, "partials", __func__));
        TRY(writes.add(it.norm_out, 4, k, "norm_out", __func__));
        TRY(writes.add(it.scale_out, 4, k, "scale_out", __func__));
        G.rep[k] = NormRep{it.grads, reinterpret_cast<const unsigned long long*>(it.table), it.skip, it.max_norm, it.partials,
                           it.norm_out, it.scale_out};
    }
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("train_grad_norm", s, 0.0, (double)K * (total * 4 + blocks * 16));
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3((unsigned)blocks, K), dim3(256), 0, s, G);
    TRY(launched(__func__));
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(K), dim3(256), 0, s, G);
    return launched(__func__);
}

int rsaf_cnnlstm_pack_params_group(const rsaf_cnnlstm_pack_item* items_host, int K, int input_dim, int channels, int hidden,
                                   int num_classes, int lstm_layers, rsaf_stream_t stream) {
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, ACT_SILU};
    PackGroup G{};
    int64_t blocks = 0, total = 0;
    TRY(seg_prepare(d, items_host, K, __func__, &G.t, &blocks, &total));
    for (int k = 0; k < K; ++k) {
        const rsaf_cnnlstm_pack_item& it = items_host[k];
        if (!(it.table && it.params)) return fail(RSAF_ERR_ARG, __func__, k, "NULL pointer");
        if (reinterpret_cast<uintptr_t>(it.params) & 15) return fail(RSAF_ERR_ARG, __func__, k, "params must be 16-byte aligned");
        for (int j = 0; j < k; ++j)
            if (overlap(items_host[j].params, total, it.params, total))
                return fail(RSAF_ERR_ARG, __func__, k, ("shares `params` with item " + std::to_string(j)).c_str());
        G.rep[k] = PackRep{reinterpret_cast<const unsigned long long*>(it.table), it.params};
    }
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("train_pack", s, 0.0, (double)K * total * 4 * 2);
    hipLaunchKernelGGL(pack_group_kernel, dim3((unsigned)blocks, K), dim3(256), 0, s, G);
    return launched(__func__);
}

int rsaf_bn_running_stats_group(const rsaf_bn_running_item* items_host, int K, int channels, rsaf_stream_t stream) {
    TRY(check_group_args(K, items_host, __func__));
    RSAF_CHECK_ARG(channels >= 1 && channels <= 1024, "channels must be in [1, 1024]");
    BnRunGroup g{};
    for (int k = 0; k < K; ++k) {
        const rsaf_bn_running_item& it = items_host[k];
        if (!it.stats) return fail(RSAF_ERR_ARG, __func__, k, "NULL pointer");
        g.item[k].stats = it.stats;
        for (int i = 0; i < 5; ++i) {
            if (it.running_mean[i] && !it.running_var[i]) return fail(RSAF_ERR_ARG, __func__, k, "running_mean without running_var");
            g.item[k].mean[i] = it.running_mean[i]; g.item[k].var[i] = it.running_var[i];
            g.item[k].momentum[i] = it.momentum[i]; g.item[k].unbias[i] = it.unbias[i];
        }
    }
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("train_bn_running", s, 0.0, (double)K * 5 * channels * 4 * 6);
    hipLaunchKernelGGL(bn_running_group_kernel, dim3((channels + 255) / 256, 5, K), dim3(256), 0, s, g, channels);
    return launched(__func__);
}

}  // extern "C"
