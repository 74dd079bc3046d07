// How the CNN-LSTM entries (cnnlstm.hip, cnnlstm_train.hip, cnnlstm_optim.hip) check their arguments and fail: the part of
// cnnlstm_layout.h's company that needs rsaf_last_error.  TRY, fail and overlap are short names for use inside
// rsaf::cnnlstm / rsaf::cnntrain, not a public interface.
#pragma once
#include "cnnlstm_layout.h"
#include "gemm_f32.h"      // Act; rsaf_common.h

namespace rsaf {
namespace cnnlstm {

static_assert(DIMS_ACT_GELU == ACT_GELU && DIMS_ACT_SILU == ACT_SILU, "dims_problem tests Act");

inline int check_dims(const Dims& d, int c_max) {
    const char* problem = dims_problem(d, c_max);
    RSAF_CHECK_ARG(!problem, problem);
    return RSAF_OK;
}

#define TRY(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)

// `who`: the entry that was called; idx < 0: a message about the call, not about one item
inline int fail(int code, const char* who, int idx, const std::string& msg) {
    set_error(std::string(who) + ": " + (idx >= 0 ? "item " + std::to_string(idx) + ": " : std::string()) + msg);
    return code;
}

// the two checks that every group entry opens with; `max_name`: how the entry's documentation calls the limit
inline int check_group_args(int K, const void* items_host, const char* who, const char* max_name = "rsaf_cnnlstm_train_group_max") {
    if (!(K >= 1 && K <= RSAF_CNNLSTM_GROUP_MAX)) return fail(RSAF_ERR_ARG, who, -1, std::string("K must be in [1, 16] (") + max_name + ")");
    if (!items_host) return fail(RSAF_ERR_ARG, who, -1, "items_host is NULL");
    return RSAF_OK;
}

// the byte ranges that the items of one group call write, two per item at most: no two may overlap (NULL: nothing written)
struct WrittenRanges {
    struct Range { const char* p; int64_t bytes; int item; const char* what; };
    Range r[RSAF_CNNLSTM_GROUP_MAX * 2];
    int n = 0;
    int add(const void* q, int64_t bytes, int k, const char* what, const char* who) {
        const char* p = reinterpret_cast<const char*>(q);
        if (!p) return RSAF_OK;
        for (int i = 0; i < n; ++i)
            if (p < r[i].p + r[i].bytes && r[i].p < p + bytes)
                return fail(RSAF_ERR_ARG, who, k, std::string("`") + what + "` overlaps `" + r[i].what + "` of item " + std::to_string(r[i].item));
        r[n++] = Range{p, bytes, k, what};
        return RSAF_OK;
    }
};

// [a, a + na) and [b, b + nb) share a float
inline bool overlap(const float* a, int64_t na, const float* b, int64_t nb) { return a < b + nb && b < a + na; }

}  // namespace cnnlstm

// the training side: the same names, the dims under the training cap on cnn_out_channels
namespace cnntrain {
using namespace cnnlstm;
inline int check_dims(const Dims& d) { return cnnlstm::check_dims(d, TRAIN_C_MAX); }
}  // namespace cnntrain

}  // namespace rsaf
