// What the inference path (cnnlstm.hip) and the training step (cnnlstm_train.hip) of the CNN-LSTM classifier call in each
// other's files and in cnnlstm_lstm.hip, which holds every recurrence kernel: a kernel is launched only from the file that
// defines it (the loss and optimizer side, cnnlstm_optim.hip, uses none of these).
#pragma once
#include "rsaf_common.h"

namespace rsaf {

// Persistent bidirectional LSTM recurrence over xproj[B][T][2][4H] (input projections + bias, gate order i,f,g,o)
// with whh[2][4H][H]; hout[B][T][2H].  With gates_save/c_save (training) the post-activation gates are stored in the
// xproj layout (gates_save may alias xproj) and the cell states in the hout layout.  Up to RSAF_CNNLSTM_GROUP_MAX independent
// recurrences (own weights, own B and T) run in ONE launch of the 4-row kernel: every B at or under the threshold, and all
// of them save gates / cell states or none does.  The descriptors travel by value in the kernel arguments; a mixed group
// (replicas of different architecture) carries an H per recurrence.
struct LstmRecItem {
    const float* xproj;
    const float* whh;
    float* hout;
    float* gates_save;
    float* c_save;
    int B, T;
};
struct LstmRecGroup { LstmRecItem item[RSAF_CNNLSTM_GROUP_MAX]; };
struct LstmRecMixedItem { LstmRecItem rec; int H; };
struct LstmRecMixedGroup { LstmRecMixedItem item[RSAF_CNNLSTM_GROUP_MAX]; };

// The BPTT recurrences in the same forms.  `gates`: the saved post-activation gates, overwritten with the pre-activation gate
// gradients; cst: the saved cell states; dh: the gradient w.r.t. the layer's output.
struct LstmBwdItem {
    float* gates;
    const float* cst;
    const float* dh;
    const float* whh;
    int B, T;
};
struct LstmBwdGroup { LstmBwdItem item[RSAF_CNNLSTM_GROUP_MAX]; };
struct LstmBwdMixedItem { LstmBwdItem rec; int H; };
struct LstmBwdMixedGroup { LstmBwdMixedItem item[RSAF_CNNLSTM_GROUP_MAX]; };

// One layer's recurrences of the K forwards / replicas of an entry.  SINGLE: one launch each.  GROUPED (one H), MIXED (an H
// per item): one launch carries those whose batch runs on the 4-row kernel, behind the own launches of the items above
// the threshold (RSAF_LSTM_SMALL_MAX).  all_or_none (the training GROUPED entries): any batch above it makes the layer SINGLE for all.
enum { SINGLE = 0, GROUPED = 1, MIXED = 2 };
int launch_lstm_rec_layer(const LstmRecMixedItem* items, int K, int mode, bool all_or_none, hipStream_t s);
int launch_lstm_bwd_layer(const LstmBwdMixedItem* items, int K, int mode, bool all_or_none, hipStream_t s);

// max_pool1d(2) over time, channels-last (cnnlstm.hip); grid, profiler scope and the launch error are the caller's
void launch_pool2(const float* x, float* y, int B, int T, int Tp, int C, int blocks, hipStream_t s);

// k = 3 / pad = 1 convolution over channels-last sequences on the exact-fp32 GEMM (cnnlstm.hip): y = act(conv(x) + bias + R)
int conv3(const float* x, const float* wk, const float* bias, const float* R, int64_t ldr, int64_t sR, float* y, int B, int T,
          int Cin, int Cout, int act, hipStream_t s, const char* tag);

// Attention pooling + classifier, the head of the inference forward, with group forms like the recurrences' (cnnlstm.hip).
// seq [B][T][2H]; pooled_out may be NULL.
struct AttnPoolItem {
    const float* seq;
    const float* watt;
    const float* batt;
    const float* wfc;
    const float* bfc;
    float* logits;
    float* pooled_out;
    int B, T;
};
struct AttnPoolGroup { AttnPoolItem item[RSAF_CNNLSTM_GROUP_MAX]; };
struct AttnPoolMixedItem { AttnPoolItem head; int H; };
struct AttnPoolMixedGroup { AttnPoolMixedItem item[RSAF_CNNLSTM_GROUP_MAX]; };

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the vector-memory counter, i.e. waits for
// the write acknowledgements of the per-step global stores of the recurrences - a few hundred cycles on every time step
// for data no other wave of the workgroup reads.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0); vmcnt / expcnt left alone
    __builtin_amdgcn_s_barrier();
}

// Drain the vector-memory counter once in front of a persistent loop: the waitcnt pass merges the loop pre-header with
// the back edge, and loads still pending from the pre-header would otherwise force vmcnt(0) in every iteration.
__device__ __forceinline__ void vmem_drain() { __builtin_amdgcn_s_waitcnt(0x0f70); }   // vmcnt(0) only

}  // namespace rsaf
