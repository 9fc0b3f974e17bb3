// tune_rules_check.cpp -- the create-time rules of shim/tune.hpp (tests/test_tune_rules.py builds this with ASan + UBSan and runs it).  No device and no
// HIP header: the rules are functions of times.  Each is run next to the expressions it replaced -- kept below as they stood inside the five timing
// loops of shim/launch.hpp and in vector_args -- over every combination of times from a set that holds the untimed value, a tie, the 0.95 guard's
// edge and the float just under it, and must give the same choice and the same bits in tune_ms / pack_ms.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "shim/tune.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++failures <= 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                    \
    } while (0)

static bool same_bits(const float *a, const float *b, int n) { return memcmp(a, b, sizeof(float) * (size_t) n) == 0; }

// ------------------------------------------------------------------------------------ the expressions before tune.hpp
static int old_vector(const float *tmin, int ncand, float tune_ms[3])
{
    constexpr int kCand = 5;
    const int cand[kCand] = {VEC_TILE_D4, VEC_TILE_D4_NOPRE, VEC_TILE_D2, VEC_TILE_D2_NOPRE, VEC_PIPE};
    float best = 1e30f;
    int best_c = VEC_AUTO;
    for (int k = 0; k < kCand - 1; ++k) {
        if (tmin[k] < best) { best = tmin[k]; best_c = cand[k]; }
    }
    if (ncand == kCand && tmin[kCand - 1] < 0.95f * best) { best = tmin[kCand - 1]; best_c = VEC_PIPE; }
    tune_ms[0] = tmin[0] < tmin[1] ? tmin[0] : tmin[1];
    tune_ms[1] = tmin[2] < tmin[3] ? tmin[2] : tmin[3];
    tune_ms[2] = ncand == kCand ? tmin[4] : 0.f;
    return best_c;
}

// returns pk_depth of the kept planes, 0 where they are freed
static int old_packed(const float *tmin, const float *tune_ms, float pack_ms[2])
{
    const int depth[3] = {0, 4, 2};
    float plain_best = tmin[0];
    for (int k = 0; k < 2; ++k) if (tune_ms[k] > 0 && tune_ms[k] < plain_best) plain_best = tune_ms[k];
    const int best = tmin[2] < tmin[1] ? 2 : 1;
    pack_ms[0] = plain_best;
    pack_ms[1] = tmin[best];
    if (!(tmin[best] < 0.95f * plain_best)) return 0;
    return depth[best];
}

static int old_blocked(const float *tmin, float tune_ms[2])
{
    constexpr int kForms = 2;
    int best = 0;
    for (int f = 0; f < kForms; ++f) { tune_ms[f] = tmin[f]; if (tmin[f] < tmin[best]) best = f; }
    return best;
}

static int old_rows(const float *tmin) { return tmin[1] < tmin[0] ? 2 : 4; }

// vector_args: kernel (0 pipe, 1 tile, 2 rows), steps in flight and PRE for option vector_form = v (or the measured form)
struct OldArgs { int kernel = 0, depth = 4; bool pre = true; };
static OldArgs old_vector_args(bool rows, int v, int rows_depth, bool f64, int vt_tiles, bool tile_default)
{
    OldArgs a;
    if (rows) {
        a.kernel = 2;
        a.depth = rows_depth ? rows_depth : (f64 ? 4 : 2);
        if (v == VEC_TILE_D2 || v == VEC_TILE_D2_NOPRE) a.depth = 2;
        if (v == VEC_TILE_D4 || v == VEC_TILE_D4_NOPRE) a.depth = 4;
    } else {
        const bool tile_forced = v == VEC_TILE_D2 || v == VEC_TILE_D4 || v == VEC_TILE_D8 || v == VEC_TILE_D4_NOPRE || v == VEC_TILE_D2_NOPRE;
        if (vt_tiles > 0 && v != VEC_PIPE && (tile_default || tile_forced)) {
            a.kernel = 1;
            a.depth = v == VEC_TILE_D2 || v == VEC_TILE_D2_NOPRE ? 2 : v == VEC_TILE_D8 ? 8 : v == VEC_TILE_D4 || v == VEC_TILE_D4_NOPRE ? 4 : (f64 ? 4 : 2);
            a.pre = v != VEC_TILE_D4_NOPRE && v != VEC_TILE_D2_NOPRE;
        }
    }
    return a;
}

int main()
{
    // untimed, a time, the guard's edge for it (not a win), the float just under the edge (a win), a clear win, an event pair that measured nothing
    const float edge = 0.95f * 1.0f;
    const float times[] = {1e30f, 1.0f, edge, std::nextafterf(edge, 0.0f), 0.5f, 0.0f};
    constexpr int N = sizeof times / sizeof *times;
    long cases = 0;

    for (int ncand = 4; ncand <= 5; ++ncand)
        for (int i = 0; i < N * N * N * N * N; ++i) {
            float t[5];
            for (int k = 0, r = i; k < 5; ++k, r /= N) t[k] = times[r % N];
            float a[3] = {-1, -1, -1}, b[3] = {-2, -2, -2};
            const int ca = old_vector(t, ncand, a), cb = vector_rule(t, ncand, b);
            CHECK(ca == cb && same_bits(a, b, 3), "vector ncand=%d t={%g %g %g %g %g}: %d {%g %g %g} != %d {%g %g %g}", ncand, t[0], t[1], t[2], t[3], t[4], ca, a[0], a[1], a[2], cb, b[0],
                  b[1], b[2]);
            ++cases;
        }

    for (int i = 0; i < N * N * N * N * N; ++i) {
        float t[3], tune[2];
        int r = i;
        for (int k = 0; k < 3; ++k, r /= N) t[k] = times[r % N];
        for (int k = 0; k < 2; ++k, r /= N) tune[k] = times[r % N];
        float a[2] = {-1, -1}, b[2] = {-2, -2};
        const int da = old_packed(t, tune, a), best = packed_rule(t, tune, b);
        const int db = best ? vec_form(kPackedCand[best])->depth : 0; // as build_packed_values reads it
        CHECK(da == db && same_bits(a, b, 2), "packed t={%g %g %g} tune={%g %g}: %d {%g %g} != %d {%g %g}", t[0], t[1], t[2], tune[0], tune[1], da, a[0], a[1], db, b[0], b[1]);
        ++cases;
    }

    for (int i = 0; i < N * N; ++i) {
        const float t[2] = {times[i % N], times[i / N]};
        float a[2] = {-1, -1}, b[2] = {-2, -2};
        const int fa = old_blocked(t, a), fb = blocked_rule(t, b);
        CHECK(fa == fb && same_bits(a, b, 2), "blocked t={%g %g}: %d != %d", t[0], t[1], fa, fb);
        const int ra = old_rows(t), rb = vec_form(kRowsCand[rows_rule(t)])->depth; // as autotune_rows reads it
        CHECK(ra == rb, "rows t={%g %g}: %d != %d", t[0], t[1], ra, rb);
        cases += 2;
    }

    // the candidates, rounds and guard of the races
    const int vcand[5] = {VEC_TILE_D4, VEC_TILE_D4_NOPRE, VEC_TILE_D2, VEC_TILE_D2_NOPRE, VEC_PIPE};
    CHECK(kVectorCands == 5 && memcmp(kVectorCand, vcand, sizeof vcand) == 0, "vector candidates");
    CHECK(kPackedCands == 3 && kPackedCand[0] == VEC_AUTO && vec_form(kPackedCand[1])->depth == 4 && vec_form(kPackedCand[2])->depth == 2, "packed candidates");
    CHECK(kRowsCands == 2 && vec_form(kRowsCand[0])->depth == 4 && vec_form(kRowsCand[1])->depth == 2, "rows candidates");
    CHECK(kBlockedForms == 2 && kVectorRounds == 3 && kPackedRounds == 3 && kBlockedRounds == 4 && kRowsRounds == 2, "round counts");
    CHECK(kClearWin == 0.95f && kNotTimed == 1e30f, "guard");

    // the form table against vector_args' comparisons: every code, both value sizes, with and without tiles, staged or not, every measured depth
    for (int v = 0; v <= 15; ++v)
        for (int f64 = 0; f64 <= 1; ++f64) {
            for (int tiles = 0; tiles <= 1; ++tiles)
                for (int tile_default = 0; tile_default <= 1; ++tile_default) {
                    const OldArgs a = old_vector_args(false, v, 0, f64, tiles, tile_default);
                    const VecForm f = vector_form_of(v, f64, tiles > 0, tile_default);
                    CHECK((a.kernel == 1) == f.tile && a.depth == f.depth && a.pre == f.pre, "form %d f64=%d tiles=%d default=%d: {%d %d %d} != {%d %d %d}", v, f64, tiles, tile_default,
                          a.kernel, a.depth, a.pre, f.tile, f.depth, f.pre);
                    ++cases;
                }
            for (int measured = 0; measured <= 4; measured += 2) {
                const OldArgs a = old_vector_args(true, v, measured, f64, 1, true);
                CHECK(a.depth == rows_depth_of(v, measured, f64), "rows form %d f64=%d measured=%d: %d != %d", v, f64, measured, a.depth, rows_depth_of(v, measured, f64));
                ++cases;
            }
        }
    // spmv_shim_info: the rows kernel's measured depth in the tile forms' codes
    CHECK(vec_code(true, 2, true) == VEC_TILE_D2 && vec_code(true, 4, true) == VEC_TILE_D4, "vec_code");
    for (const VecForm &f : kVecForms) CHECK(vec_code(f.tile, f.depth, f.pre) == f.code && vec_form(f.code) == &f, "table round trip %d", f.code);

    printf("tune rules: %ld cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
