// Kernels of the CNN-LSTM classifier shared by the inference path (cnnlstm.hip) and the training step
// (cnnlstm_train.hip; its loss and optimizer side is cnnlstm_optim.hip and uses none of these).
#pragma once
#include "rsaf_common.h"

namespace rsaf {

// Persistent bidirectional LSTM recurrence over xproj[B][T][2][4H] (input projections + bias, gate order i,f,g,o)
// with whh[2][4H][H]; hout[B][T][2H].  With gates_save/c_save (training) the post-activation gates are stored in the
// xproj layout (gates_save may alias xproj) and the cell states in the hout layout.
int launch_lstm_rec(const float* xproj, const float* whh, float* hout, float* gates_save, float* c_save, int B, int T,
                    int H, hipStream_t s);

// The same for up to RSAF_CNNLSTM_GROUP_MAX independent recurrences of one H (own weights, own B and T) in ONE launch of the
// 4-row kernel: every B must be <= lstm_small_max(), and all of them save gates / cell states or none does.  The
// descriptors travel by value in the kernel arguments.
struct LstmRecItem {
    const float* xproj;
    const float* whh;
    float* hout;
    float* gates_save;
    float* c_save;
    int B, T;
};
struct LstmRecGroup {
    LstmRecItem item[RSAF_CNNLSTM_GROUP_MAX];
};
int launch_lstm_rec_group(const LstmRecItem* items, int K, int H, hipStream_t s);

// The same for recurrences of different H (mixed groups: replicas of different architecture) in ONE launch of 512-thread
// workgroups.  An H = 128 item runs as above, grid.y its direction.  The workgroup of an H = 64 item runs BOTH directions of
// its tile, waves 0-3 direction 0 and waves 4-7 direction 1, each half on LDS buffers of its own: the halves loop over the
// same T, so all eight waves meet at every barrier, and the grid.y == 1 workgroups of such an item leave whole.  No
// workgroup ever has some of its waves returned while others wait at a barrier.
struct LstmRecMixedItem {
    LstmRecItem rec;
    int H;
};
struct LstmRecMixedGroup {
    LstmRecMixedItem item[RSAF_CNNLSTM_GROUP_MAX];
};
int launch_lstm_rec_group_mixed(const LstmRecMixedItem* items, int K, hipStream_t s);

// Attention pooling + classifier (the head of the inference forward) of up to RSAF_CNNLSTM_GROUP_MAX independent forwards of
// one H and one num_classes in ONE launch; the descriptors travel by value in the kernel arguments.  seq [B][T][2H];
// pooled_out may be NULL.
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
struct AttnPoolGroup {
    AttnPoolItem item[RSAF_CNNLSTM_GROUP_MAX];
};
// the heads of forwards of different H (one num_classes) in ONE launch
struct AttnPoolMixedItem {
    AttnPoolItem head;
    int H;
};
struct AttnPoolMixedGroup {
    AttnPoolMixedItem item[RSAF_CNNLSTM_GROUP_MAX];
};

// Largest batch that runs on the 4-row recurrence kernels (environment RSAF_LSTM_SMALL_MAX, read once; default 1 024).
int lstm_small_max();

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
