// What the two halves of the CNN-LSTM training step share: the model step (cnnlstm_train.hip: forward and backward) and
// the optimizer side (cnnlstm_optim.hip: cross-entropy, Adam, gradient norm, blob packing, BatchNorm running statistics).
// That is the dims and their checks, the layout of the parameter / gradient blob, and how an entry fails.  Only those two
// files include it: TRY, fail and overlap are short names for use inside rsaf::cnntrain, not a public interface.
#pragma once
#include "gemm_f32.h"      // Act; rsaf_common.h

namespace rsaf {
namespace cnntrain {

struct Dims {
    int D, C, H, NC, L, act;
};

inline int64_t pad4(int64_t n) { return (n + 3) & ~int64_t(3); }
inline int64_t pad32(int64_t n) { return (n + 31) & ~int64_t(31); }

// ---- parameter / gradient blob ---------------------------------------------------------------------------
struct ConvP {
    int64_t w, b, g, be;
};
struct PLayout {
    ConvP c1, sc, c2, c3, c4;
    int64_t wih[4], bsum[4], whh[4];
    int64_t watt, batt, wfc, bfc, total;
};

inline PLayout make_playout(const Dims& d) {
    PLayout L{};
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t s = o; o += pad4(n); return s; };
    auto conv = [&](int taps, int cin) { ConvP c; c.w = take((int64_t)d.C * taps * cin); c.b = take(d.C); c.g = take(d.C); c.be = take(d.C); return c; };
    L.c1 = conv(3, d.D);
    if (d.D != d.C) L.sc = conv(1, d.D); else L.sc = ConvP{-1, -1, -1, -1};
    L.c2 = conv(3, d.C); L.c3 = conv(3, d.C); L.c4 = conv(3, d.C);
    for (int l = 0; l < d.L; ++l) {
        const int in = l == 0 ? d.C : 2 * d.H;
        L.wih[l] = take((int64_t)8 * d.H * in);
        L.bsum[l] = take(8 * d.H);
        L.whh[l] = take((int64_t)2 * 4 * d.H * d.H);
    }
    L.watt = take(2 * d.H); L.batt = take(1);
    L.wfc = take((int64_t)d.NC * 2 * d.H); L.bfc = take(d.NC);
    L.total = o;
    return L;
}

// what is wrong with the dims, or NULL
inline const char* dims_problem(const Dims& d) {
    if (!(d.D > 0 && d.D % 4 == 0)) return "input_dim must be a positive multiple of 4";
    if (!(d.C > 0 && d.C % 4 == 0 && d.C <= 1024)) return "cnn_out_channels must be a multiple of 4 in [4, 1024]";
    if (!(d.H == 64 || d.H == 128)) return "lstm_hidden_dim must be 64 or 128 (reference search space)";
    if (!(d.NC >= 1 && d.NC <= 16)) return "num_classes must be in [1, 16]";
    if (!(d.L >= 1 && d.L <= 4)) return "lstm_layers must be in [1, 4]";
    if (!(d.act == ACT_GELU || d.act == ACT_SILU)) return "activation must be gelu (1) or silu (2)";
    return nullptr;
}

inline int check_dims(const Dims& d) {
    const char* problem = dims_problem(d);
    RSAF_CHECK_ARG(!problem, problem);
    return RSAF_OK;
}

#define TRY(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)

// `who`: the entry that was called; idx < 0: a message about the call, not about one item
inline int fail(int code, const char* who, int idx, const char* msg) {
    set_error(std::string(who) + ": " + (idx >= 0 ? "item " + std::to_string(idx) + ": " : std::string()) + msg);
    return code;
}

// the two checks that every group entry opens with
inline int check_group_args(int K, const void* items_host, const char* who) {
    if (!(K >= 1 && K <= RSAF_CNNLSTM_GROUP_MAX)) return fail(RSAF_ERR_ARG, who, -1, "K must be in [1, 16] (rsaf_cnnlstm_train_group_max)");
    if (!items_host) return fail(RSAF_ERR_ARG, who, -1, "items_host is NULL");
    return RSAF_OK;
}

inline bool overlap(const float* a, int64_t na, const float* b, int64_t nb) { return a < b + nb && b < a + na; }

}  // namespace cnntrain
}  // namespace rsaf
