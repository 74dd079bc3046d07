// The sizes of the MSHDS voice analyses as the library computed them before they moved into mshds_voice_layout.h: the
// expressions of rsaf_mshds_resample10k (LDS request), rsaf_mshds_resample10k_table_stride and pulses_layout, copied
// verbatim but for the names of the function arguments.  Included by voice_layout_replay.cpp.
namespace parent {

constexpr int RS_QL = 4;
constexpr int RS_QT = 64 * RS_QL;

inline int table_stride(int depth) { return (2 * depth + 1 + 8 * (RS_QL - 1) + 7) / 8 * 8 + 8; }

inline size_t resample_lds_bytes(int depth) {
    const int taps = 2 * depth + 1;
    const int span = 8 * (RS_QT - 1) + 8 + taps + 8 * RS_QL + 8;       // phase bases differ by < 8; the tap loop runs past `taps`
    const size_t lds = (size_t)(span + span / 32 + 2) * sizeof(double);
    return lds;
}

// sizeof(Stretch) = 16, sizeof(int2) = 8, sizeof(double2) = 16
inline void pulses_layout(int n_clips, int max_frames, double pitch_dt, double ceiling, int* max_st, int* cap_slots, int64_t* total) {
    *max_st = max_frames / 2 + 2;
    *cap_slots = (int)((double)max_frames * pitch_dt * ceiling * 1.25) + 4 * *max_st + 16;
    *total = (int64_t)n_clips * ((int64_t)*max_st * (16 + 8) + sizeof(int) * 2 + sizeof(double) +
                                 (int64_t)*cap_slots * (16 + sizeof(double))) + 256;
}

}  // namespace parent
