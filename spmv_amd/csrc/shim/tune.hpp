// shim/tune.hpp -- the create-time choices as data and pure functions of the measured times: the CSR-vector forms as one table, every race's candidates and
// rounds (shim/launch.hpp: race_forms), and what is done with the minimum time per candidate.  No HIP and no handle in here: a host program compiles this
// header alone (tests/c/tune_rules_check.cpp).  All arithmetic is float, like hipEventElapsedTime's times.
#pragma once

// Kernel forms of the CSR-vector schedule; the codes are public (option vector_form, spmv_hip_info.tuned_choice).
enum { VEC_AUTO = 0, VEC_PIPE = 4, VEC_TILE_D2 = 5, VEC_TILE_D8 = 6, VEC_TILE_D4 = 10, VEC_TILE_D4_NOPRE = 11, VEC_TILE_D2_NOPRE = 12 };
struct VecForm {
    int code;
    bool tile; // the tile kernel (false: the pipe kernel)
    int depth; // steps in flight
    bool pre;  // tile kernel: step 0 issued before the barrier
};
static constexpr VecForm kVecForms[] = {{VEC_PIPE, false, 4, true},   {VEC_TILE_D2, true, 2, true},        {VEC_TILE_D8, true, 8, true},
                                        {VEC_TILE_D4, true, 4, true}, {VEC_TILE_D4_NOPRE, true, 4, false}, {VEC_TILE_D2_NOPRE, true, 2, false}};
// The form a code names (NULL: any other code -- none forced, none measured), and the code of the form with these properties (0: none)
static inline const VecForm *vec_form(int code)
{
    for (const VecForm &f : kVecForms) if (f.code == code) return &f;
    return nullptr;
}
static inline int vec_code(bool tile, int depth, bool pre)
{
    for (const VecForm &f : kVecForms) if (f.tile == tile && f.depth == depth && f.pre == pre) return f.code;
    return VEC_AUTO;
}
// The tile or pipe launch under `code` (forced, else measured): a tile form runs wherever the schedule has tiles, the pipe form wherever it is named; any
// other code runs the tile kernel where most x windows stage (tile_default), at the dtype's measured depth, PRE on.
static inline VecForm vector_form_of(int code, bool f64, bool has_tiles, bool tile_default)
{
    const VecForm *f = vec_form(code);
    if (!has_tiles || !(f ? f->tile : tile_default)) return {code, false, 4, true};
    return {code, true, f ? f->depth : (f64 ? 4 : 2), f ? f->pre : true};
}
// Steps in flight of the rows kernel: a forced tile form's two or four, else what create() measured, else the dtype's default
static inline int rows_depth_of(int code, int measured, bool f64)
{
    const VecForm *f = vec_form(code);
    return f && f->tile && f->depth <= 4 ? f->depth : measured ? measured : (f64 ? 4 : 2);
}

// The races: candidates in launch order, interleaved rounds, and the guard -- a form that costs something elsewhere (the pipe form's global gathers, the
// packed planes' memory) wins only below kClearWin x the best of the others: a noisy sample must not decide.
static constexpr float kClearWin = 0.95f, kNotTimed = 1e30f; // kNotTimed: a candidate's time before its first sample
static constexpr int kVectorCands = 5, kPackedCands = 3, kRowsCands = 2, kBlockedForms = 2;
static constexpr int kVectorCand[kVectorCands] = {VEC_TILE_D4, VEC_TILE_D4_NOPRE, VEC_TILE_D2, VEC_TILE_D2_NOPRE, VEC_PIPE}; // the pipe form last: not timed where (nearly) every tile stages
static constexpr int kPackedCand[kPackedCands] = {VEC_AUTO, VEC_TILE_D4, VEC_TILE_D2};                                       // the plain winner, then the packed kernel at these depths
static constexpr int kRowsCand[kRowsCands] = {VEC_TILE_D4, VEC_TILE_D2};                                                     // the rows kernel at these depths
static constexpr int kVectorRounds = 3, kPackedRounds = 3, kBlockedRounds = 4, kRowsRounds = 2;

// CSR-vector: the first strict minimum over the tile forms, the pipe form (timed when ncand = kVectorCands) only on a clear win -> the winner's code.
// ms[0] / ms[1]: the best time four / two steps deep, ms[2]: the pipe form's (0: not timed).
static inline int vector_rule(const float *t, int ncand, float ms[3])
{
    float best = kNotTimed;
    int code = VEC_AUTO;
    ms[0] = ms[1] = kNotTimed;
    for (int k = 0; k < kVectorCands - 1; ++k) {
        if (t[k] < best) { best = t[k]; code = kVectorCand[k]; }
        float &m = ms[vec_form(kVectorCand[k])->depth == 4 ? 0 : 1];
        if (t[k] < m) m = t[k];
    }
    const bool pipe_timed = ncand == kVectorCands;
    ms[2] = pipe_timed ? t[kVectorCands - 1] : 0.f;
    return pipe_timed && t[kVectorCands - 1] < kClearWin * best ? VEC_PIPE : code;
}
// Packed planes, t in kPackedCand's order.  The plain best is t[0] or vector_rule's own (tune_ms[0], [1]; <= 0: none), whichever is lower; pack_ms = {plain
// best, packed best} -> the packed winner's index in kPackedCand, 0 where the planes do not win clearly.
static inline int packed_rule(const float t[3], const float tune_ms[2], float pack_ms[2])
{
    float plain_best = t[0];
    for (int k = 0; k < 2; ++k) if (tune_ms[k] > 0 && tune_ms[k] < plain_best) plain_best = tune_ms[k];
    const int best = t[2] < t[1] ? 2 : 1;
    pack_ms[0] = plain_best;
    pack_ms[1] = t[best];
    return t[best] < kClearWin * plain_best ? best : 0;
}
// Blocked executor: the first strict minimum over the two forms, ms = their times.  Rows kernel: the index in kRowsCand, two deep only when strictly faster.
static inline int blocked_rule(const float t[2], float ms[2])
{
    int best = 0;
    for (int f = 0; f < kBlockedForms; ++f) { ms[f] = t[f]; if (t[f] < t[best]) best = f; }
    return best;
}
static inline int rows_rule(const float t[2]) { return t[1] < t[0] ? 1 : 0; }
