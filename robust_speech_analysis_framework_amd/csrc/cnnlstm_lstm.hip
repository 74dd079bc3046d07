// The LSTM recurrences of the CNN-LSTM classifier on gfx950, forward (SAVE: the training forward, which keeps gates and cell
// states) and BPTT, each as a 16-row kernel, a 4-row kernel for small batches and the 4-row body in a group kernel (one H) and
// a mixed group kernel (an H per recurrence).  Launchers: cnnlstm_kernels.h; the LDS of every kernel: cnnlstm_layout.h.
//
// Forward, 16 rows: one workgroup = 16 batch rows of one direction for all T' steps (rows are
// independent, so there is no inter-workgroup traffic).  H/16 waves; wave w owns hidden units
// 16w..16w+15 for all four gates, and keeps its slice of W_hh permanently in registers as
// v_mfma_f32_16x16x4_f32 B-fragments (H registers per lane).  Per step: the accumulators start from
// the prefetched input projection, h_{t-1} is read from LDS as the A operand, the gate nonlinearity
// and cell update are lane-local (all four gates of a (row, unit) pair land in the same lane and
// register index), h_t goes to LDS (double-buffered, one barrier per step) and to HBM.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "cnnlstm_kernels.h"
#include "cnnlstm_layout.h"

namespace rsaf {
namespace cnnlstm {

using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- persistent bidirectional LSTM recurrence ------------------------------------------------------
// SAVE (training): the post-activation gates overwrite the input projection in place (the lane that read an element
// is the lane that rewrites it, one step after the read of the next step was issued) and the cell state is kept.
template <int H, bool SAVE>
__global__ __launch_bounds__(H / 16 * 64) void lstm_rec_kernel(const float* xproj, const float* __restrict__ whh,
                                                               float* __restrict__ hout, float* gates_save,
                                                               float* __restrict__ c_save, int B, int T) {
    constexpr int LDH = rec_ldh(H);
    constexpr int KG = H / 16;                   // k-groups of 16 (4 MFMA k-steps each)
    __shared__ __attribute__((aligned(16))) float hbuf[2][16][LDH];
    static_assert(sizeof(hbuf) == rec_lds_floats(H) * sizeof(float), "cnnlstm_layout.h states this kernel's LDS");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = tid >> 6;
    const int col = lane & 15;
    const int q = lane >> 4;
    const int dir = blockIdx.y;
    const int b0 = blockIdx.x * 16;
    const int unit = 16 * w + col;

    // W_hh slice as B fragments: element (g, j) of gate gt holds W[gt*H + unit][16g + 4q + j]
    float breg[4][KG * 4];
    const float* wd = whh + (int64_t)dir * 4 * H * H;
#pragma unroll
    for (int gt = 0; gt < 4; ++gt)
#pragma unroll
        for (int g = 0; g < KG; ++g) {
            const float4 v = *reinterpret_cast<const float4*>(wd + (int64_t)(gt * H + unit) * H + 16 * g + 4 * q);
            breg[gt][4 * g + 0] = v.x; breg[gt][4 * g + 1] = v.y;
            breg[gt][4 * g + 2] = v.z; breg[gt][4 * g + 3] = v.w;
        }
    for (int i = tid; i < 2 * 16 * LDH; i += H / 16 * 64) (&hbuf[0][0][0])[i] = 0.0f;

    // rows of this lane in the C/D map: q*4 + r, clamped to the last batch row (copies replicate it bit for bit)
    int64_t xoff[4], hoff[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = b0 + q * 4 + r;
        const int bc = b < B ? b : B - 1;
        xoff[r] = (int64_t)bc * T * 8 * H + dir * 4 * H + unit;
        hoff[r] = (int64_t)bc * T * 2 * H + dir * H + unit;
    }
    float cst[4] = {0.f, 0.f, 0.f, 0.f};
    float xin[4][4];
    {
        const int t = dir ? T - 1 : 0;
#pragma unroll
        for (int gt = 0; gt < 4; ++gt)
#pragma unroll
            for (int r = 0; r < 4; ++r) xin[gt][r] = xproj[xoff[r] + (int64_t)t * 8 * H + gt * H];
    }
    vmem_drain();
    __syncthreads();

    int cur = 0;
    for (int s = 0; s < T; ++s) {
        const int t = dir ? T - 1 - s : s;
        f32x4 acc[4];
#pragma unroll
        for (int gt = 0; gt < 4; ++gt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[gt][r] = xin[gt][r];
        {                                          // prefetch the next step's input projection (the last step reloads
            const int tn = s + 1 < T ? (dir ? t - 1 : t + 1) : t;      // its own: the loop body stays branch-free)
#pragma unroll
            for (int gt = 0; gt < 4; ++gt)
#pragma unroll
                for (int r = 0; r < 4; ++r) xin[gt][r] = xproj[xoff[r] + (int64_t)tn * 8 * H + gt * H];
        }
#pragma unroll
        for (int g = 0; g < KG; ++g) {
            const float4 a4 = *reinterpret_cast<const float4*>(&hbuf[cur][col][16 * g + 4 * q]);
            const float a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int gt = 0; gt < 4; ++gt)
                    acc[gt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], breg[gt][4 * g + j], acc[gt], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float ig = sigmoidf_(acc[0][r]);
            const float fg = sigmoidf_(acc[1][r]);
            const float gg = tanhf(acc[2][r]);
            const float og = sigmoidf_(acc[3][r]);
            cst[r] = fg * cst[r] + ig * gg;
            const float hv = og * tanhf(cst[r]);
            hbuf[cur ^ 1][q * 4 + r][unit] = hv;
            // rows past B are clamped to row B-1 and replicate it bit for bit: their stores rewrite the same values, and
            // leaving them unconditional keeps the loop branch-free (exact vmcnt bookkeeping, no store drain per step)
            hout[hoff[r] + (int64_t)t * 2 * H] = hv;
            if (SAVE) {
                float* gs = gates_save + xoff[r] + (int64_t)t * 8 * H;
                gs[0] = ig; gs[H] = fg; gs[2 * H] = gg; gs[3 * H] = og;
                c_save[hoff[r] + (int64_t)t * 2 * H] = cst[r];
            }
        }
        lds_barrier();
        cur ^= 1;
    }
}

// ---- the same recurrence for small batches: 4 batch rows per workgroup -------------------------------------
// With a handful of sequences (the reference trains with batches of 4 and 8, src/dl_cv_strategies.py:234,265) the
// 16-row tile above wastes 3/4 of its MFMA work and leaves the step time at 16 rows' worth.  Here a workgroup owns 4
// rows of one direction and uses v_mfma_f32_4x4x1_16B_f32 (16 independent 4x4 outer products per instruction): row i
// of every block is batch row i, the 64 (block, j) columns of wave w are the four gates of hidden units 16w..16w+15
// (column c = 16*gate + u).  W_hh stays register-resident (H registers per lane: the lane's column over all k), h
// is broadcast from LDS.  The gate pre-activations of one (row, unit) land in four lanes (one per gate); they are
// exchanged through a wave-private LDS tile so that lane (q, u) updates cell (row q, unit u).
// The body is shared by the one-recurrence kernel and the group kernel below: `dir` and `tile` (the 4-row tile of the
// batch) are what blockIdx.y / blockIdx.x are to the former.
// HALVES = 2 (the mixed group kernel, H = 64): the workgroup is two such bodies side by side, threads [0, 16 H) and
// [16 H, 32 H), each on its own half of the LDS buffers; `dir` is then the half's own direction.  Both halves take the
// same B and T, so they meet at every barrier.
template <int H, bool SAVE, int HALVES = 1>
__device__ __forceinline__ void lstm_rec4_body(const float* xproj, const float* __restrict__ whh,
                                               float* __restrict__ hout, float* gates_save,
                                               float* __restrict__ c_save, int B, int T, int dir, int tile) {
    constexpr int LDH = rec_ldh(H);
    constexpr int NW = H / 16;
    __shared__ __attribute__((aligned(16))) float hbuf_all[HALVES][2][4][LDH];
    __shared__ float gx_all[HALVES][NW][4][REC4_GX_LD];   // [wave][row][16*gate + u], row stride 80: conflict-free both ways
    static_assert(sizeof(hbuf_all) + sizeof(gx_all) == rec4_lds_floats(H, HALVES) * sizeof(float), "cnnlstm_layout.h states this body's LDS");
    const int half = HALVES == 1 ? 0 : (int)threadIdx.x / (NW * 64);
    auto& hbuf = hbuf_all[half];
    auto& gx = gx_all[half];
    const int tid = HALVES == 1 ? (int)threadIdx.x : (int)threadIdx.x - half * (NW * 64), lane = tid & 63, w = tid >> 6;
    const int gq = lane >> 4, u = lane & 15;        // as a column: gate gq of unit u; as a cell owner: row gq of unit u
    const int b0 = tile * 4;
    const int unit = 16 * w + u;

    float breg[H];
    {
        const float* wr = whh + (int64_t)dir * 4 * H * H + (int64_t)(gq * H + unit) * H;
#pragma unroll
        for (int k = 0; k < H; k += 4) {
            const float4 v = *reinterpret_cast<const float4*>(wr + k);
            breg[k] = v.x; breg[k + 1] = v.y; breg[k + 2] = v.z; breg[k + 3] = v.w;
        }
    }
    for (int i = tid; i < 2 * 4 * LDH; i += NW * 64) (&hbuf[0][0][0])[i] = 0.0f;

    // as a column: input projections of rows 0..3; as a cell owner: outputs of row gq
    int64_t xoff[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int bc = min(b0 + r, B - 1);
        xoff[r] = (int64_t)bc * T * 8 * H + dir * 4 * H + gq * H + unit;
    }
    const int bo = min(b0 + gq, B - 1);
    const int64_t hoff = (int64_t)bo * T * 2 * H + dir * H + unit;
    const int64_t goff = (int64_t)bo * T * 8 * H + dir * 4 * H + unit;
    const int arow = lane & 3;                      // A operand: lane 4*blk + i carries batch row i
    const float ya = gq == 2 ? 2.0f : 1.0f, yb = gq == 2 ? -2.0f : -1.0f, yc = gq == 2 ? -1.0f : 0.0f;
    float cst = 0.f;
    float xin[4];
    {
        const int t = dir ? T - 1 : 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) xin[r] = xproj[xoff[r] + (int64_t)t * 8 * H];
    }
    vmem_drain();
    __syncthreads();

    int cur = 0;
    for (int s = 0; s < T; ++s) {
        const int t = dir ? T - 1 - s : s;
        f32x4 acc[4];
        acc[0] = f32x4{xin[0], xin[1], xin[2], xin[3]};
#pragma unroll
        for (int a = 1; a < 4; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
        {
            const int tn = s + 1 < T ? (dir ? t - 1 : t + 1) : t;      // branch-free: the last step reloads its own row
#pragma unroll
            for (int r = 0; r < 4; ++r) xin[r] = xproj[xoff[r] + (int64_t)tn * 8 * H];
        }
        // h in batches of 8 float4 (32 k), the next batch in flight while this one feeds the matrix pipe
        float4 ab[2][8];
#pragma unroll
        for (int j = 0; j < 8; ++j) ab[0][j] = *reinterpret_cast<const float4*>(&hbuf[cur][arow][4 * j]);
#pragma unroll
        for (int kb = 0; kb < H / 32; ++kb) {
            if (kb + 1 < H / 32) {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    ab[(kb + 1) & 1][j] = *reinterpret_cast<const float4*>(&hbuf[cur][arow][32 * (kb + 1) + 4 * j]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float4 a4 = ab[kb & 1][j];
                const int k = 32 * kb + 4 * j;
                acc[0] = __builtin_amdgcn_mfma_f32_4x4x1f32(a4.x, breg[k + 0], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_4x4x1f32(a4.y, breg[k + 1], acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_4x4x1f32(a4.z, breg[k + 2], acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_4x4x1f32(a4.w, breg[k + 3], acc[3], 0, 0, 0);
            }
        }
        // gate nonlinearity in the column's lane (one gate type per lane: y = ya / (1 + exp(yb * x)) + yc is the
        // logistic function for i, f, o and tanh for g), then the 4x4 exchange through the wave's LDS tile
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float pre = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
            gx[w][r][lane] = ya * __builtin_amdgcn_rcpf(1.0f + __expf(yb * pre)) + yc;
        }
        __builtin_amdgcn_wave_barrier();
        const float ig = gx[w][gq][u], fg = gx[w][gq][16 + u], gg = gx[w][gq][32 + u], og = gx[w][gq][48 + u];
        cst = fg * cst + ig * gg;
        const float hv = og * (2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(-2.0f * cst)) - 1.0f);
        hbuf[cur ^ 1][gq][unit] = hv;
        hout[hoff + (int64_t)t * 2 * H] = hv;          // rows past B replicate row B-1 (see lstm_rec_kernel)
        if (SAVE) {
            float* gs = gates_save + goff + (int64_t)t * 8 * H;
            gs[0] = ig; gs[H] = fg; gs[2 * H] = gg; gs[3 * H] = og;
            c_save[hoff + (int64_t)t * 2 * H] = cst;
        }
        lds_barrier();
        cur ^= 1;
    }
}

template <int H, bool SAVE>
__global__ __launch_bounds__(H / 16 * 64) void lstm_rec4_kernel(const float* xproj, const float* __restrict__ whh,
                                                                float* __restrict__ hout, float* gates_save,
                                                                float* __restrict__ c_save, int B, int T) {
    lstm_rec4_body<H, SAVE>(xproj, whh, hout, gates_save, c_save, B, T, blockIdx.y, blockIdx.x);
}

// Several independent recurrences (same H; own weights, own B and T) in one launch: grid (max tiles, 2, K), blockIdx.z
// selects the descriptor.  The descriptors are kernel arguments (wave-uniform: they load through scalar registers), so
// a launch needs no device table and no copy.  A workgroup whose tile lies beyond its recurrence's batch leaves before
// it touches LDS or a barrier; the others loop over their own T.
template <int H, bool SAVE>
__global__ __launch_bounds__(H / 16 * 64) void lstm_rec4_group_kernel(const LstmRecGroup g) {
    const LstmRecItem& it = g.item[blockIdx.z];
    if ((int)blockIdx.x * 4 >= it.B) return;
    lstm_rec4_body<H, SAVE>(it.xproj, it.whh, it.hout, it.gates_save, it.c_save, it.B, it.T, blockIdx.y, blockIdx.x);
}

// Recurrences of different H in one launch (LstmRecMixedItem, cnnlstm_kernels.h): grid (max tiles, 2, K), 512 threads.  Every
// exit below is taken by the whole workgroup (the descriptor and the block index are uniform) and comes before the first
// LDS access or barrier; a workgroup that enters a body runs all eight waves through every barrier of its loop.
template <bool SAVE>
__global__ __launch_bounds__(512) void lstm_rec4_group_mixed_kernel(const LstmRecMixedGroup g) {
    const LstmRecMixedItem& m = g.item[blockIdx.z];
    const LstmRecItem& it = m.rec;
    if ((int)blockIdx.x * 4 >= it.B) return;
    if (m.H == 128) {
        lstm_rec4_body<128, SAVE>(it.xproj, it.whh, it.hout, it.gates_save, it.c_save, it.B, it.T, blockIdx.y, blockIdx.x);
        return;
    }
    if (blockIdx.y != 0) return;                       // H = 64: the blockIdx.y == 0 workgroup runs both directions
    const int dir = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8);
    lstm_rec4_body<64, SAVE, 2>(it.xproj, it.whh, it.hout, it.gates_save, it.c_save, it.B, it.T, dir, blockIdx.x);
}

// ---- persistent LSTM backward recurrence (BPTT) ---------------------------------------------------------------------
// One workgroup = 16 batch rows of one direction; wave w owns hidden units 16w..16w+15.  Walks the time steps in the
// reverse of the forward order.  Per step, lane-local: dh = dh_out + dh_rec, gate/cell derivatives from the saved
// post-activation gates and cell states; the pre-activation gate gradients overwrite the saved gates (they are the
// operand of the weight / input gradients afterwards) and go to LDS as the MFMA A operand of
//     dh_rec[row][unit] = sum_k dgates[row][k] * W_hh[k][unit],   k over the 4H gate rows,
// with W_hh register-resident as B fragments (H registers per lane).
template <int H>
__global__ __launch_bounds__(H / 16 * 64) void lstm_bwd_kernel(float* gates, const float* __restrict__ cst,
                                                               const float* __restrict__ dh_out, const float* __restrict__ whh,
                                                               int B, int T) {
    constexpr int LDG = bwd_ldg(H);
    constexpr int KG = 4 * H / 16;                  // k-groups of 16 gate rows
    extern __shared__ __attribute__((aligned(16))) float dgbuf[];     // [2][16][LDG]: bwd_lds_floats(H), requested by launch_lstm_bwd
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, col = lane & 15, q = lane >> 4;
    const int dir = blockIdx.y, b0 = blockIdx.x * 16, unit = 16 * w + col;

    // B fragments: breg[4g + j] = W_hh[dir][16g + 4q + j][unit]
    float breg[KG * 4];
    const float* wd = whh + (int64_t)dir * 4 * H * H;
#pragma unroll
    for (int g = 0; g < KG; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) breg[4 * g + j] = wd[(int64_t)(16 * g + 4 * q + j) * H + unit];
    for (int i = tid; i < bwd_lds_floats(H); i += H / 16 * 64) dgbuf[i] = 0.0f;

    int brow[4];
    int64_t goff[4], hoff[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = b0 + q * 4 + r;
        brow[r] = b < B;
        const int bc = b < B ? b : B - 1;
        goff[r] = (int64_t)bc * T * 8 * H + dir * 4 * H + unit;
        hoff[r] = (int64_t)bc * T * 2 * H + dir * H + unit;
    }
    float dcc[4] = {0.f, 0.f, 0.f, 0.f};            // dL/dc carried to the previous forward step
    f32x4 acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();

    int cur = 0;
    for (int s = 0; s < T; ++s) {
        const int t = dir ? s : T - 1 - s;           // reverse of the forward order
        const int tprev = dir ? t + 1 : t - 1;       // the step the forward pass ran just before t
        const bool first = dir ? (t == T - 1) : (t == 0);
        float* dgw = dgbuf + (cur ^ 1) * 16 * LDG;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* gp = gates + goff[r] + (int64_t)t * 8 * H;
            const float ig = gp[0], fg = gp[H], gg = gp[2 * H], og = gp[3 * H];
            const float c = cst[hoff[r] + (int64_t)t * 2 * H];
            const float cpl = cst[hoff[r] + (int64_t)(first ? t : tprev) * 2 * H];
            const float cp = first ? 0.f : cpl;
            const float dh = dh_out[hoff[r] + (int64_t)t * 2 * H] + (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
            const float tc = tanhf(c);
            const float dc = dcc[r] + dh * og * (1.0f - tc * tc);
            const float d_o = dh * tc * og * (1.0f - og);
            const float d_i = dc * gg * ig * (1.0f - ig);
            const float d_f = dc * cp * fg * (1.0f - fg);
            const float d_g = dc * ig * (1.0f - gg * gg);
            dcc[r] = dc * fg;
            const int row = q * 4 + r;
            dgw[row * LDG + unit] = d_i; dgw[row * LDG + H + unit] = d_f;
            dgw[row * LDG + 2 * H + unit] = d_g; dgw[row * LDG + 3 * H + unit] = d_o;
            // rows past B are clamped copies of row B-1: they must NOT store here, because this loop reads the gates of
            // step t row by row and a copy in an earlier register row would overwrite them before the real row reads
            if (brow[r]) {
                float* go = gates + goff[r] + (int64_t)t * 8 * H;
                go[0] = d_i; go[H] = d_f; go[2 * H] = d_g; go[3 * H] = d_o;
            }
        }
        lds_barrier();
        cur ^= 1;
        const float* dgr = dgbuf + cur * 16 * LDG;
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < KG; ++g) {
            const float4 a4 = *reinterpret_cast<const float4*>(&dgr[col * LDG + 16 * g + 4 * q]);
            acc[g & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, breg[4 * g + 0], acc[g & 3], 0, 0, 0);
            acc[g & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, breg[4 * g + 1], acc[g & 3], 0, 0, 0);
            acc[g & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, breg[4 * g + 2], acc[g & 3], 0, 0, 0);
            acc[g & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, breg[4 * g + 3], acc[g & 3], 0, 0, 0);
        }
    }
}

// ---- the same backward recurrence for small batches: 4 batch rows per workgroup ---------------------------------------
// Wave w owns hidden units 16w..16w+15; lane (q, u) = (lane / 16, lane % 16) owns cell (row q, unit 16w + u): lane-local
// gate / cell derivatives, dgates to HBM (in place) and to LDS (double-buffered: one LDS-only barrier per step).
// dh_rec = dgates . W_hh with v_mfma_f32_4x4x1_16B_f32 (row i of every block = batch row i): the 16 blocks of an
// instruction are 4 gates x 4 groups of 4 units, i.e. lane (g, u) contracts the H rows of gate g against unit u (its
// W_hh column slice is register-resident, H registers) and a two-step butterfly over the gate lanes completes the sum
// in a fixed order.  No partial products through LDS.
// The body is shared by the one-recurrence kernel and the group kernels below (`dir`, `tile`: direction and 4-row tile).
// HALVES = 2 (the mixed group kernel, H = 64): two such bodies side by side in one workgroup, threads [0, 16 H) and
// [16 H, 32 H), each on its own half of the LDS buffer and with its own `dir`, as lstm_rec4_body does it.
template <int H, int HALVES = 1>
__device__ __forceinline__ void lstm_bwd4_body(float* gates, const float* __restrict__ cst, const float* __restrict__ dh_out,
                                               const float* __restrict__ whh, int B, int T, int dir, int tile) {
    constexpr int NW = H / 16;
    constexpr int LDG = bwd4_ldg(H);                // row stride = 20 banks (mod 32): the four rows of a fragment read and the
                                                    // 16-lane row groups of the cell owners' writes land on distinct banks
    __shared__ __attribute__((aligned(16))) float dg_all[HALVES][2][4][LDG];
    static_assert(sizeof(dg_all) == bwd4_lds_floats(H, HALVES) * sizeof(float), "cnnlstm_layout.h states this body's LDS");
    const int half = HALVES == 1 ? 0 : (int)threadIdx.x / (NW * 64);
    auto& dg = dg_all[half];
    const int tid = HALVES == 1 ? (int)threadIdx.x : (int)threadIdx.x - half * (NW * 64), lane = tid & 63, w = tid >> 6;
    const int q = lane >> 4, u = lane & 15;
    const int b0 = tile * 4;
    const int unit = 16 * w + u;
    const int arow = lane & 3;

    // breg[m] = W_hh[dir][q*H + m][unit]   (q as the gate of this lane's blocks)
    float breg[H];
    {
        const float* wd = whh + (int64_t)dir * 4 * H * H + (int64_t)(q * H) * H + unit;
#pragma unroll
        for (int m = 0; m < H; ++m) breg[m] = wd[(int64_t)m * H];
    }
    const int bo = min(b0 + q, B - 1);              // rows past B replicate row B-1 bit for bit (see lstm_rec_kernel)
    const int64_t goff = (int64_t)bo * T * 8 * H + dir * 4 * H + unit;
    const int64_t hoff = (int64_t)bo * T * 2 * H + dir * H + unit;
    float dcc = 0.f, dh_rec = 0.f;
    float ig, fg, gg, og, cc, dho;                  // operands of the current step (prefetched)
    {
        const int t = dir ? 0 : T - 1;
        const float* gp = gates + goff + (int64_t)t * 8 * H;
        ig = gp[0]; fg = gp[H]; gg = gp[2 * H]; og = gp[3 * H];
        cc = cst[hoff + (int64_t)t * 2 * H];
        dho = dh_out[hoff + (int64_t)t * 2 * H];
    }
    vmem_drain();
    int cur = 0;
    for (int s = 0; s < T; ++s) {
        const int t = dir ? s : T - 1 - s;           // reverse of the forward order
        const int tprev = dir ? t + 1 : t - 1;       // the step the forward pass ran just before t == the next step here
        const bool last = s + 1 == T;
        // next step's operands (branch-free: the last step reloads its own and zeroes c_prev)
        const int tl = last ? t : tprev;
        const float* gp = gates + goff + (int64_t)tl * 8 * H;
        const float nig = gp[0], nfg = gp[H], ngg = gp[2 * H], nog = gp[3 * H];
        const float ncl = cst[hoff + (int64_t)tl * 2 * H];
        const float ncc = last ? 0.f : ncl;
        const float ndho = dh_out[hoff + (int64_t)tl * 2 * H];

        const float dh = dho + dh_rec;
        const float tc = 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(-2.0f * cc)) - 1.0f;
        const float dc = dcc + dh * og * (1.0f - tc * tc);
        const float d_o = dh * tc * og * (1.0f - og);
        const float d_i = dc * gg * ig * (1.0f - ig);
        const float d_f = dc * ncc * fg * (1.0f - fg);           // c of the previous forward step (0 at the first)
        const float d_g = dc * ig * (1.0f - gg * gg);
        dcc = dc * fg;
        float* dgw = &dg[cur][q][0];
        dgw[unit] = d_i; dgw[H + unit] = d_f; dgw[2 * H + unit] = d_g; dgw[3 * H + unit] = d_o;
        {
            float* go = gates + goff + (int64_t)t * 8 * H;
            go[0] = d_i; go[H] = d_f; go[2 * H] = d_g; go[3 * H] = d_o;
        }
        lds_barrier();
        // A operand: lane 4*blk + i carries batch row i; the block's gate is this lane's q
        const float* dgr = &dg[cur][arow][q * H];
        f32x4 acc[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
        float4 ab[2][8];
#pragma unroll
        for (int j = 0; j < 8; ++j) ab[0][j] = *reinterpret_cast<const float4*>(dgr + 4 * j);
#pragma unroll
        for (int kb = 0; kb < H / 32; ++kb) {
            if (kb + 1 < H / 32) {
#pragma unroll
                for (int j = 0; j < 8; ++j) ab[(kb + 1) & 1][j] = *reinterpret_cast<const float4*>(dgr + 32 * (kb + 1) + 4 * j);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float4 a4 = ab[kb & 1][j];
                const int m = 32 * kb + 4 * j;
                acc[0] = __builtin_amdgcn_mfma_f32_4x4x1f32(a4.x, breg[m + 0], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_4x4x1f32(a4.y, breg[m + 1], acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_4x4x1f32(a4.z, breg[m + 2], acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_4x4x1f32(a4.w, breg[m + 3], acc[3], 0, 0, 0);
            }
        }
        // lane (g, u), register r: sum over the rows of gate g for (batch row r, unit u).  Butterfly over g; lane (q, u)
        // keeps batch row q.
        float pr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            pr[r] = v;
        }
        dh_rec = q == 0 ? pr[0] : q == 1 ? pr[1] : q == 2 ? pr[2] : pr[3];
        cur ^= 1;
        ig = nig; fg = nfg; gg = ngg; og = nog; cc = ncc; dho = ndho;
    }
}

template <int H>
__global__ __launch_bounds__(H / 16 * 64) void lstm_bwd4_kernel(float* gates, const float* __restrict__ cst,
                                                                const float* __restrict__ dh_out, const float* __restrict__ whh,
                                                                int B, int T) {
    lstm_bwd4_body<H>(gates, cst, dh_out, whh, B, T, blockIdx.y, blockIdx.x);
}

// The BPTT recurrences of several independent replicas in one launch, as lstm_rec4_group_kernel runs the forward ones.

template <int H>
__global__ __launch_bounds__(H / 16 * 64) void lstm_bwd4_group_kernel(const LstmBwdGroup g) {
    const LstmBwdItem& it = g.item[blockIdx.z];
    if ((int)blockIdx.x * 4 >= it.B) return;
    lstm_bwd4_body<H>(it.gates, it.cst, it.dh, it.whh, it.B, it.T, blockIdx.y, blockIdx.x);
}

// BPTT recurrences of different H in one launch, as lstm_rec4_group_mixed_kernel runs the forward ones (same exits).

__global__ __launch_bounds__(512) void lstm_bwd4_group_mixed_kernel(const LstmBwdMixedGroup g) {
    const LstmBwdMixedItem& m = g.item[blockIdx.z];
    const LstmBwdItem& it = m.rec;
    if ((int)blockIdx.x * 4 >= it.B) return;
    if (m.H == 128) {
        lstm_bwd4_body<128>(it.gates, it.cst, it.dh, it.whh, it.B, it.T, blockIdx.y, blockIdx.x);
        return;
    }
    if (blockIdx.y != 0) return;
    const int dir = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8);
    lstm_bwd4_body<64, 2>(it.gates, it.cst, it.dh, it.whh, it.B, it.T, dir, blockIdx.x);
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
// f(H, SAVE) with both as compile-time constants
template <class F>
static void with_h_save(int H, bool save, F f) {
    using std::integral_constant;
    if (save) { if (H == 128) f(integral_constant<int, 128>{}, std::true_type{}); else f(integral_constant<int, 64>{}, std::true_type{}); }
    else { if (H == 128) f(integral_constant<int, 128>{}, std::false_type{}); else f(integral_constant<int, 64>{}, std::false_type{}); }
}

// what a group kernel's argument takes of an item: a mixed group all of it, a group of one H the recurrence
template <class M> static const M& member_of(const M& m, const M&) { return m; }
template <class M, class I> static const I& member_of(const M& m, const I&) { return m.rec; }

// the descriptors of a group launch into the kernel argument, the grid over the largest batch of 4-row tiles and the flops of
// all of them; launch(g, grid) runs inside the profiler scope.  The caller asks for the launch error.
template <class Group, class MixedItem, class Launch>
static void launch_gathered(const char* family, const MixedItem* items, int K, hipStream_t s, Launch launch) {
    Group g{};
    int tiles = 0;
    double flops = 0.0;
    for (int k = 0; k < K; ++k) {
        g.item[k] = member_of(items[k], g.item[k]);
        tiles = std::max(tiles, (items[k].rec.B + 3) / 4);
        flops += 2.0 * items[k].rec.B * items[k].rec.T * 2.0 * 4 * items[k].H * items[k].H;
    }
    ProfScope prof(family, s, flops, 0.0);
    launch(g, dim3(tiles, 2, K));
}

}  // namespace cnnlstm

using namespace cnnlstm;

// Largest batch that runs on the 4-row recurrence kernels (environment RSAF_LSTM_SMALL_MAX, read once; default 1 024).
static int lstm_small_max() {
    static const int v = [] { const char* e = getenv("RSAF_LSTM_SMALL_MAX"); return e ? atoi(e) : 1024; }();
    return v;
}

static int launch_lstm_rec(const LstmRecItem& it, int H, hipStream_t s) {
    const int B = it.B, T = it.T;
    RSAF_CHECK_ARG(H == 64 || H == 128, "lstm_hidden_dim must be 64 or 128");
    RSAF_CHECK_ARG((it.gates_save == nullptr) == (it.c_save == nullptr), "gates_save and c_save go together");
    ProfScope prof("lstm_recurrent", s, 2.0 * B * T * 2.0 * 4 * H * H, 0.0);
    // 4-row workgroups while they still fit the chip about twice over; the 16-row tile beyond (same pipe time for 4x the rows)
    const bool small = B <= lstm_small_max();
    dim3 grid(small ? (B + 3) / 4 : (B + 15) / 16, 2);
    with_h_save(H, it.gates_save != nullptr, [&](auto h, auto save) {
        constexpr int HH = decltype(h)::value;
        constexpr bool SV = decltype(save)::value;
        if (small) hipLaunchKernelGGL((lstm_rec4_kernel<HH, SV>), grid, dim3(HH / 16 * 64), 0, s, it.xproj, it.whh, it.hout, it.gates_save, it.c_save, B, T);
        else hipLaunchKernelGGL((lstm_rec_kernel<HH, SV>), grid, dim3(HH / 16 * 64), 0, s, it.xproj, it.whh, it.hout, it.gates_save, it.c_save, B, T);
    });
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

// one H for all (the items' own H is the same)
static int launch_lstm_rec_group(const LstmRecMixedItem* items, int K, int H, hipStream_t s) {
    RSAF_CHECK_ARG(H == 64 || H == 128, "lstm_hidden_dim must be 64 or 128");
    RSAF_CHECK_ARG(items && K >= 1 && K <= RSAF_CNNLSTM_GROUP_MAX, "a group holds 1 to 16 recurrences");
    const bool save = items[0].rec.gates_save != nullptr;
    for (int k = 0; k < K; ++k) {
        const LstmRecItem& it = items[k].rec;
        RSAF_CHECK_ARG(it.B >= 1 && it.B <= lstm_small_max() && it.T >= 1, "a grouped recurrence runs on the 4-row tiles");
        RSAF_CHECK_ARG((it.gates_save != nullptr) == save && (it.c_save != nullptr) == save,
                       "gates_save and c_save go together, for all recurrences of a group or for none");
    }
    with_h_save(H, save, [&](auto h, auto sv) {
        constexpr int HH = decltype(h)::value;
        launch_gathered<LstmRecGroup>("lstm_recurrent", items, K, s, [&](const LstmRecGroup& g, dim3 grid) {
            hipLaunchKernelGGL((lstm_rec4_group_kernel<HH, decltype(sv)::value>), grid, dim3(HH / 16 * 64), 0, s, g);
        });
    });
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

static int launch_lstm_rec_group_mixed(const LstmRecMixedItem* items, int K, hipStream_t s) {
    RSAF_CHECK_ARG(items && K >= 1 && K <= RSAF_CNNLSTM_GROUP_MAX, "a group holds 1 to 16 recurrences");
    const bool save = items[0].rec.gates_save != nullptr;
    for (int k = 0; k < K; ++k) {
        const LstmRecItem& it = items[k].rec;
        const int H = items[k].H;
        RSAF_CHECK_ARG(H == 64 || H == 128, "lstm_hidden_dim must be 64 or 128");
        RSAF_CHECK_ARG(it.B >= 1 && it.B <= lstm_small_max() && it.T >= 1, "a grouped recurrence runs on the 4-row tiles");
        RSAF_CHECK_ARG((it.gates_save != nullptr) == save && (it.c_save != nullptr) == save,
                       "gates_save and c_save go together, for all recurrences of a group or for none");
    }
    launch_gathered<LstmRecMixedGroup>("lstm_recurrent", items, K, s, [&](const LstmRecMixedGroup& g, dim3 grid) {
        if (save) hipLaunchKernelGGL(lstm_rec4_group_mixed_kernel<true>, grid, dim3(512), 0, s, g);
        else hipLaunchKernelGGL(lstm_rec4_group_mixed_kernel<false>, grid, dim3(512), 0, s, g);
    });
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

static int launch_lstm_bwd(const LstmBwdItem& it, int H, hipStream_t s) {
    const int B = it.B, T = it.T;
    ProfScope prof("lstm_bwd_recurrent", s, 2.0 * B * T * 2.0 * 4 * H * H, 0.0);
    if (B <= lstm_small_max()) {
        dim3 grid((B + 3) / 4, 2);
        if (H == 128) hipLaunchKernelGGL(lstm_bwd4_kernel<128>, grid, dim3(512), 0, s, it.gates, it.cst, it.dh, it.whh, B, T);
        else hipLaunchKernelGGL(lstm_bwd4_kernel<64>, grid, dim3(256), 0, s, it.gates, it.cst, it.dh, it.whh, B, T);
    } else {
        dim3 grid((B + 15) / 16, 2);
        const size_t lds = (size_t)bwd_lds_floats(H) * sizeof(float);
        if (H == 128)                                       // the one request above 64 KiB
            RSAF_CHECK_HIP(hipFuncSetAttribute((const void*)lstm_bwd_kernel<128>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        if (H == 128) hipLaunchKernelGGL(lstm_bwd_kernel<128>, grid, dim3(512), lds, s, it.gates, it.cst, it.dh, it.whh, B, T);
        else hipLaunchKernelGGL(lstm_bwd_kernel<64>, grid, dim3(256), lds, s, it.gates, it.cst, it.dh, it.whh, B, T);
    }
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

// the BPTT group launchers take every B <= lstm_small_max() and every H 64 or 128 (launch_layer; the entries' checks)
static int launch_lstm_bwd_group(const LstmBwdMixedItem* items, int K, int H, hipStream_t s) {
    launch_gathered<LstmBwdGroup>("lstm_bwd_recurrent", items, K, s, [&](const LstmBwdGroup& g, dim3 grid) {
        if (H == 128) hipLaunchKernelGGL(lstm_bwd4_group_kernel<128>, grid, dim3(512), 0, s, g);
        else hipLaunchKernelGGL(lstm_bwd4_group_kernel<64>, grid, dim3(256), 0, s, g);
    });
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

static int launch_lstm_bwd_group_mixed(const LstmBwdMixedItem* items, int K, hipStream_t s) {
    launch_gathered<LstmBwdMixedGroup>("lstm_bwd_recurrent", items, K, s, [&](const LstmBwdMixedGroup& g, dim3 grid) {
        hipLaunchKernelGGL(lstm_bwd4_group_mixed_kernel, grid, dim3(512), 0, s, g);
    });
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

// ---- one layer of an entry: which recurrences share the group launch --------------------------------------------------------
// single | group | mixed: the three launchers of one direction of time
template <class Item, class MixedItem>
static int launch_layer(const MixedItem* items, int K, int mode, bool all_or_none, hipStream_t s, int (*single)(const Item&, int, hipStream_t),
                        int (*group)(const MixedItem*, int, int, hipStream_t), int (*mixed)(const MixedItem*, int, hipStream_t)) {
    if (mode == GROUPED && all_or_none)
        for (int k = 0; k < K; ++k)
            if (items[k].rec.B > lstm_small_max()) mode = SINGLE;
    MixedItem small[RSAF_CNNLSTM_GROUP_MAX];
    int n = 0;
    for (int k = 0; k < K; ++k) {
        if (mode == SINGLE || items[k].rec.B > lstm_small_max()) { int rc = single(items[k].rec, items[k].H, s); if (rc) return rc; }
        else small[n++] = items[k];
    }
    if (n && mode == MIXED) return mixed(small, n, s);
    if (n) return group(small, n, items[0].H, s);
    return RSAF_OK;
}

int launch_lstm_rec_layer(const LstmRecMixedItem* items, int K, int mode, bool all_or_none, hipStream_t s) {
    return launch_layer(items, K, mode, all_or_none, s, launch_lstm_rec, launch_lstm_rec_group, launch_lstm_rec_group_mixed);
}

int launch_lstm_bwd_layer(const LstmBwdMixedItem* items, int K, int mode, bool all_or_none, hipStream_t s) {
    return launch_layer(items, K, mode, all_or_none, s, launch_lstm_bwd, launch_lstm_bwd_group, launch_lstm_bwd_group_mixed);
}

}  // namespace rsaf
