// tests/leaf_host/leaf_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_leaf_shortcut.py compiles and runs it).
//
// The leaf shortcut (forge3d_amd/csrc/f3d_trace.h leaf_shortcut) against the full leaf solve, on the host: every leaf handed
// to leaf_finish is solved with the shortcut off and on, and any disagreement -- the verdict, or a bit of t_hit -- ends the
// program with a non-zero status.  For any-hit leaves the verdict-only form is checked too: the same verdict, and a t_hit that
// answers `t < min(tmax, 1e30)` as the full path's does.
//
//   leaf_harness synthetic [millions]   set (i): synthetic (dv0, dv1, dv2, t0, t1), default 200 million
//   leaf_harness march <mini_dem.npy>   set (ii): every leaf the real marches queue on the golden DEM
//
// Built as a program (its own main; may be built with -fsanitize=address,undefined) and, by the pytest file, as a shared
// library next to the emulator's entry points: leaf_tap_counts() reports what each test settled in an emulator render.
#include "../emul/f3d_emul.cpp"

#include <atomic>
#include <cinttypes>
#include <omp.h>

namespace {

std::atomic<unsigned long long> g_settled[2][4];  // [any_hit][kLeafFull .. kLeafCross]
std::atomic<unsigned long long> g_checked{0}, g_bad{0};
thread_local bool t_in_tap = false;

uint32_t bits_of(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

void report(const char *what, const RayCtx &r, const float *dv, float t0, float t1, bool any_hit) {
    g_bad.fetch_add(1);
    fprintf(stderr, "DISAGREE %s: dv %a %a %a  t0 %a t1 %a  any_hit %d  tmin %a tmax %a\n", what, dv[0], dv[1], dv[2], t0, t1,
            (int)any_hit, r.tmin, r.tmax);
    if (!leaf_tap()) _Exit(1);  // the program: the first disagreement ends it (a library's caller reads leaf_tap_counts)
}

// Both paths on one leaf.  Returns what leaf_shortcut says of it.
int check_leaf(const RayCtx &r, const float *dv, float t0, float t1, bool any_hit) {
    const float untouched = f_from_bits(0x7fc0beefu);
    int &force = leaf_shortcut_force();
    const int before = force;
    float t_off = untouched, t_on = untouched, t_v = untouched;
    force = 0;
    const bool h_off = leaf_finish<false>(r, dv, t0, t1, any_hit, t_off);
    force = 1;
    const bool h_on = leaf_finish<false>(r, dv, t0, t1, any_hit, t_on);
    if (h_on != h_off || bits_of(t_on) != bits_of(t_off)) report("full result", r, dv, t0, t1, any_hit);
    if (any_hit) {
        const bool h_v = leaf_finish<true>(r, dv, t0, t1, true, t_v);
        const bool want = h_off && t_off < r.tmax && t_off < 1e30f, got = h_v && t_v < r.tmax && t_v < 1e30f;
        if (h_v != h_off || want != got || (h_v && !(t_v > r.tmin))) report("verdict", r, dv, t0, t1, true);
    }
    force = before;
    g_checked.fetch_add(1, std::memory_order_relaxed);
    // (the coefficients as leaf_finish forms them)
    const float c = dv[0], a = 2.0f * dv[2] + 2.0f * dv[0] - 4.0f * dv[1], b = dv[2] - dv[0] - a;
    if (any_hit && c <= 0.0f) return -1;
    return leaf_shortcut(a, b, c, dv[2], t0, t1, r.tmin, r.tmax);
}

void tap(const RayCtx &r, const float *dv, float t0, float t1, bool any_hit, bool) {
    if (t_in_tap) return;
    t_in_tap = true;
    const int kind = check_leaf(r, dv, t0, t1, any_hit);
    if (kind >= 0) g_settled[any_hit ? 1 : 0][kind].fetch_add(1, std::memory_order_relaxed);
    t_in_tap = false;
}

// ---- set (i) ------------------------------------------------------------------------------------------------------------
struct Rng {
    uint64_t s;
    uint64_t next() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return s;
    }
    float uni() { return (float)(next() >> 40) * (1.0f / 16777216.0f); }  // [0, 1)
    float sym() { return 2.0f * uni() - 1.0f; }
    uint32_t below(uint32_t n) { return (uint32_t)((next() >> 33) % n); }
};

float step_ulps(float f, int k) {  // k floats up (or down) in the ordering of the finite floats
    if (f != f) return f;
    int32_t i = (int32_t)bits_of(f);
    i = i < 0 ? (int32_t)0x80000000u - i : i;  // monotone integer
    i += k;
    const uint32_t u = i < 0 ? 0x80000000u - (uint32_t)i : (uint32_t)i;
    return f_from_bits(u);
}
int32_t ordinal(float f) {
    const int32_t i = (int32_t)bits_of(f);
    return i < 0 ? (int32_t)0x80000000u - i : i;
}
float from_ordinal(int32_t i) { return f_from_bits(i < 0 ? 0x80000000u - (uint32_t)i : (uint32_t)i); }

struct Leaf {
    float dv[3], t0, t1;
};
RayCtx ray_of(float tmin, float tmax) {
    RayCtx r{};
    r.o = V3{0.0f, 0.0f, 0.0f};
    r.d = V3{0.0f, 1.0f, 0.0f};
    r.tmin = tmin;
    r.tmax = tmax;
    return r;
}
void both(const RayCtx &r, const Leaf &l) {
    check_leaf(r, l.dv, l.t0, l.t1, false);
    check_leaf(r, l.dv, l.t0, l.t1, true);
}

// The thresholds of leaf_shortcut as predicates of a leaf: each family walks one input until the predicate flips between
// two neighbouring floats and solves the leaves on both sides of the flip (and every leaf probed on the way).
bool predicate(int which, const Leaf &l) {
    const float c = l.dv[0], a = 2.0f * l.dv[2] + 2.0f * l.dv[0] - 4.0f * l.dv[1], b = l.dv[2] - l.dv[0] - a;
    switch (which) {
        case 0: return b > 4.0f * f_abs(a);
        case 1: return c < 1e15f;
        case 2: return leaf_less_margin(f_min(c, -l.dv[2]), f_abs(a), b, c) > 0.0f;
        case 3: return leaf_less_margin(f_min(c, l.dv[2]) - 0.25f * f_max(a, 0.0f), f_abs(a), b, c) > 0.0f;
        case 4: return b + c > kLeafTau * c;
        default: return f_abs(a) >= 1e-12f;
    }
}
void walk_to_flip(int which, int slot, Leaf l, const RayCtx &r, float other_end) {
    float *x = slot < 3 ? &l.dv[slot] : slot == 3 ? &l.t0 : &l.t1;
    int32_t lo = ordinal(*x), hi = ordinal(other_end);
    const bool at_lo = predicate(which, l);
    *x = other_end;
    both(r, l);
    if (predicate(which, l) == at_lo) return;  // no flip between the ends
    while ((int64_t)hi - lo > 1 || (int64_t)lo - hi > 1) {
        const int32_t mid = (int32_t)(((int64_t)lo + hi) / 2);
        *x = from_ordinal(mid);
        both(r, l);
        if (predicate(which, l) == at_lo) lo = mid;
        else hi = mid;
    }
    for (int k = -3; k <= 3; k++) {
        *x = from_ordinal(lo + k);
        both(r, l);
    }
}

const float kSpecial[] = {0.0f, -0.0f, 1e-45f, -1e-45f, 1e-40f, 3e-39f, 1e-38f, 1e-30f, 1.0000001e-30f, -1e-30f, 1e-12f, 9.9999e-13f,
                          -1e-12f, 1e-3f, 1.0f, -1.0f, 4000.0f, 1e6f, 1.0000001e6f, 1e15f, 1.0000001e15f, 1e18f, -1e18f, 2e19f, 1e30f,
                          1.0000001e30f, 2e30f, -1e30f, 3e38f, -3e38f, __builtin_inff(), -__builtin_inff(), __builtin_nanf("")};
constexpr int kSpecials = (int)(sizeof(kSpecial) / sizeof(kSpecial[0]));

void synthetic(unsigned long long total) {
    // every combination of special values in the three clearances, at ordinary and at special parameters
    {
        const RayCtx rays[] = {ray_of(1e-3f, 1e30f), ray_of(0.0f, 100.0f), ray_of(-1.0f, 3e38f), ray_of(1e-3f, __builtin_inff())};
#pragma omp parallel for schedule(dynamic, 1)
        for (int i = 0; i < kSpecials; i++)
            for (int j = 0; j < kSpecials; j++)
                for (int k = 0; k < kSpecials; k++)
                    for (const RayCtx &r : rays) {
                        both(r, Leaf{{kSpecial[i], kSpecial[j], kSpecial[k]}, 1.0f, 2.0f});
                        both(r, Leaf{{kSpecial[i], kSpecial[j], kSpecial[k]}, 2.0f, 2.0f});
                        both(r, Leaf{{kSpecial[i], kSpecial[j], kSpecial[k]}, 1e-3f, 49.9f});
                    }
#pragma omp parallel for schedule(dynamic, 1)
        for (int i = 0; i < kSpecials; i++)  // ... and in the two parameters, over leaves of each kind
            for (int j = 0; j < kSpecials; j++)
                for (const RayCtx &r : rays) {
                    both(r, Leaf{{1.0f, 0.1f, -1.0f}, kSpecial[i], kSpecial[j]});
                    both(r, Leaf{{1.0f, 2.0f, 3.5f}, kSpecial[i], kSpecial[j]});
                    both(r, Leaf{{1.0f, 1.1f, 1.0f}, kSpecial[i], kSpecial[j]});
                    both(r, Leaf{{1e-3f, -0.2f, 1e-3f}, kSpecial[i], kSpecial[j]});
                }
    }
    const int threads = omp_get_max_threads();
#pragma omp parallel for schedule(static, 1)
    for (int th = 0; th < threads; th++) {
        Rng g{0x9E3779B97F4A7C15ull * (uint64_t)(th + 1)};
        while (g_checked.load(std::memory_order_relaxed) < total) {
            for (int rep = 0; rep < 4096; rep++) {
                const float scale = exp2f(-26.6f + 43.2f * g.uni());  // 1e-8 ... 1e5
                const float tmax = g.below(4) == 0 ? 50.0f + 100.0f * g.uni() : 1e30f;
                const RayCtx r = ray_of(g.below(8) == 0 ? 0.0f : 1e-3f, tmax);
                Leaf l;
                l.t0 = g.below(16) == 0 ? r.tmin : r.tmin + 40.0f * g.uni() * g.uni();
                l.t1 = g.below(16) == 0 ? l.t0 : l.t0 + 30.0f * g.uni() * g.uni();
                const uint32_t family = g.below(16);
                if (family < 5) {  // anything
                    for (float &d : l.dv) d = scale * g.sym();
                } else if (family < 8) {  // nearly straight: a is small against b and c
                    const float c = scale * g.sym(), slope = scale * g.sym(), bend = scale * g.sym() * exp2f(-24.0f * g.uni());
                    l.dv[0] = c;
                    l.dv[1] = c + 0.5f * slope + bend;
                    l.dv[2] = c + slope;
                } else if (family < 11) {  // heights of thousands of metres, clearances of millimetres: a is rounding noise
                    const float ulp = 4000.0f * 1.1920929e-7f, c = 1e-3f * (0.2f + 4.0f * g.uni());
                    const float slope = g.below(3) == 0 ? 0.0f : 30.0f * g.sym() * g.uni();
                    l.dv[0] = g.below(4) == 0 ? c : c + ulp * (float)((int)g.below(9) - 4);
                    l.dv[1] = c + 0.5f * slope + ulp * (float)((int)g.below(9) - 4);
                    l.dv[2] = c + slope + ulp * (float)((int)g.below(9) - 4);
                } else if (family < 13) {  // exact small integers times a power of two: a = 0, b = 4 |a|, ties of every kind
                    const float unit = exp2f((float)((int)g.below(60) - 40));
                    for (float &d : l.dv) d = unit * (float)((int)g.below(33) - 16);
                } else if (family == 13) {  // grazing: the discriminant near zero
                    const float s = g.uni(), a = scale * g.uni(), eps = a * g.sym() * exp2f(-20.0f * g.uni());
                    const float c = a * s * s + eps, b = -2.0f * a * s;  // a (x - s)^2 + eps
                    l.dv[0] = c;
                    l.dv[1] = c + 0.5f * b + 0.25f * a;
                    l.dv[2] = c + b + a;
                } else {  // a special value in one slot of an ordinary leaf
                    for (float &d : l.dv) d = scale * g.sym();
                    const uint32_t slot = g.below(5);
                    const float v = kSpecial[g.below(kSpecials)];
                    if (slot < 3) l.dv[slot] = v;
                    else if (slot == 3) l.t0 = v;
                    else l.t1 = v;
                }
                both(r, l);
                if (g.below(8) == 0) {  // the thresholds, to the ulp, from this leaf
                    const int which = (int)g.below(8);
                    if (which < 6) {
                        const int slot = (int)g.below(3);
                        walk_to_flip(which, slot, l, r, l.dv[slot] + scale * 8.0f * g.sym());
                        walk_to_flip(which, slot, l, r, -l.dv[slot]);
                    } else if (which == 6) {
                        for (int k = -2; k <= 2; k++) {
                            Leaf m = l;
                            m.t0 = step_ulps(r.tmin, k);
                            both(r, m);
                        }
                    } else {
                        for (int k = -2; k <= 2; k++) {
                            Leaf m = l;
                            m.t1 = step_ulps((g.below(2) ? 0.5f : 1.0f) * r.tmax, k);  // (and the far end at tmax itself)
                            m.t0 = m.t1 * g.uni();
                            both(r, m);
                        }
                    }
                }
            }
        }
    }
}

// ---- set (ii) -----------------------------------------------------------------------------------------------------------
bool load_npy_f32(const char *path, std::vector<float> &data, uint32_t &w, uint32_t &h) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    unsigned char head[10];
    if (fread(head, 1, 10, f) != 10 || memcmp(head, "\x93NUMPY", 6) != 0 || head[6] != 1) return fclose(f), false;
    const size_t len = head[8] | (head[9] << 8);
    std::string text(len, ' ');
    if (fread(&text[0], 1, len, f) != len) return fclose(f), false;
    unsigned rows = 0, cols = 0;
    const size_t at = text.find("'shape': (");
    if (text.find("'<f4'") == std::string::npos || text.find("False") == std::string::npos || at == std::string::npos ||
        sscanf(text.c_str() + at, "'shape': (%u, %u", &rows, &cols) != 2)
        return fclose(f), false;
    data.resize((size_t)rows * cols);
    const bool ok = fread(data.data(), 4, data.size(), f) == data.size();
    fclose(f);
    w = cols;
    h = rows;
    return ok;
}

int march(const char *dem_path) {
    std::vector<float> dem;
    uint32_t w = 0, h = 0;
    if (!load_npy_f32(dem_path, dem, w, h)) {
        fprintf(stderr, "cannot read %s\n", dem_path);
        return 2;
    }
    const float spacing = 30.0f, ox = -0.5f * spacing * (float)(w - 1), oz = -0.5f * spacing * (float)(h - 1);
    const float exaggerations[] = {1.0f, 20.0f, 37.0f};
    unsigned long long rays_run = 0;
    for (float ex : exaggerations)
        for (int curved = 0; curved < 2; curved++) {
            Rng g{0xD1B54A32D192ED03ull + (uint64_t)(ex * 16.0f) + (uint64_t)curved};
            const uint32_t n = 16768;  // 262 waves; 6 x 16 768 > 10^5 rays
            std::vector<float> rays(8 * (size_t)n);
            for (uint32_t i = 0; i < n; i++) {
                float *r = &rays[8 * (size_t)i];
                const uint32_t ix = g.below(w - 1), iz = g.below(h - 1);
                const bool lattice = (i & 1u) != 0u;
                const float fx = lattice ? 0.0f : g.uni(), fz = lattice ? 0.0f : g.uni();
                const float ground = ex * f_max(f_max(dem[iz * w + ix], dem[iz * w + ix + 1]), f_max(dem[(iz + 1) * w + ix], dem[(iz + 1) * w + ix + 1]));
                const uint32_t kind = g.below(4);  // on the surface (secondary rays) ... high above (camera rays)
                const float lift = kind == 0 ? 1e-3f : kind == 1 ? 0.5f * g.uni() : kind == 2 ? ex * 40.0f * g.uni() : ex * 900.0f * g.uni();
                r[0] = f_fma((float)ix + fx, spacing, ox);
                r[1] = ground + lift;
                r[2] = f_fma((float)iz + fz, spacing, oz);
                r[3] = 1e-3f;
                float dx, dy, dz;
                if (lattice) {  // along the lattice's rows, columns and diagonals: corners met exactly
                    const int dirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};
                    const int *d = dirs[g.below(8)];
                    dx = (float)d[0];
                    dz = (float)d[1];
                    dy = (0.6f * g.sym()) * ex * 0.05f;
                } else {
                    dx = g.sym();
                    dz = g.sym();
                    dy = g.sym() * g.uni() * ex * 0.08f;
                }
                const float inv = 1.0f / sqrtf(dx * dx + dy * dy + dz * dz + 1e-30f);
                r[4] = dx * inv;
                r[5] = dy * inv;
                r[6] = dz * inv;
                r[7] = g.below(4) == 0 ? 200.0f + 3000.0f * g.uni() : 1e30f;
            }
            std::vector<uint32_t> hit(n);
            std::vector<float> t(n), nrm(3 * (size_t)n);
            const float k2 = curved ? 1.0f / (2.0f * 7433000.0f) : 0.0f;
            // one lane at a time: sorted descent (0 closest, 1 any), march (2 any, 3 closest; +4: start in the origin's cell)
            for (int mode : {0, 1, 2, 3, 6, 7})
                if (emul_trace_batch(dem.data(), w, h, ox, oz, spacing, spacing, ex, k2, (uint32_t)curved, rays.data(), n, mode, curved,
                                     hit.data(), t.data(), nrm.data()) != 0)
                    return 2;
            // whole waves, the ray sharing live (slices, verdict board, closest-hit sharing)
            for (int mode : {6, 3})
                for (uint32_t share : {0u, 64u})
                    if (emul_trace_batch_wave(dem.data(), w, h, ox, oz, spacing, spacing, ex, k2, (uint32_t)curved, rays.data(), n, mode, curved,
                                              share, hit.data(), t.data(), nrm.data(), nullptr) != 0)
                        return 2;
            rays_run += n;
        }
    printf("march: %llu rays on %ux%u\n", rays_run, w, h);
    return 0;
}

void print_counts() {
    for (int any = 0; any < 2; any++)
        printf("%s leaves: full %llu, miss A %llu, miss B %llu, crossing %llu\n", any ? "any-hit" : "closest-hit",
               g_settled[any][kLeafFull].load(), g_settled[any][kLeafMissA].load(), g_settled[any][kLeafMissB].load(),
               g_settled[any][kLeafCross].load());
}

}  // namespace

extern "C" {
// For the pytest file (this source built as a library): tap on / off, and what the tapped leaves were.
void leaf_tap_enable(int32_t on) {
    for (auto &row : g_settled)
        for (auto &n : row) n = 0;
    g_bad = 0;
    g_checked = 0;
    leaf_tap() = on ? tap : nullptr;
}
// out[0..3] closest-hit full / A / B / crossing, out[4..7] any-hit, out[8] disagreements
void leaf_tap_counts(unsigned long long *out) {
    for (int any = 0; any < 2; any++)
        for (int k = 0; k < 4; k++) out[4 * any + k] = g_settled[any][k].load();
    out[8] = g_bad.load();
}
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "synthetic")) {
        const unsigned long long total = 1000000ull * (argc >= 3 ? strtoull(argv[2], nullptr, 10) : 200ull);
        synthetic(total);
        printf("synthetic: %llu leaf solves checked\n", g_checked.load());
    } else if (argc >= 3 && !strcmp(argv[1], "march")) {
        leaf_tap() = tap;
        const int rc = march(argv[2]);
        leaf_tap() = nullptr;
        if (rc) return rc;
        printf("march: %llu leaf solves checked\n", g_checked.load());
        print_counts();
    } else {
        fprintf(stderr, "usage: leaf_harness synthetic [millions] | march <dem.npy>\n");
        return 2;
    }
    if (g_bad.load()) {
        fprintf(stderr, "%llu disagreements\n", g_bad.load());
        return 1;
    }
    return 0;
}
