// scene_prep.cpp -- scene_prep.h's arithmetic and the C ABI's entry points
// that need no device (include/nori_gpu.h: nori_scene_*, nori_film_*, ..;
// those that start from the scene's tree are in scene_plan.cpp).
#include "scene_prep.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rebuild.h"

namespace nori {

std::string &last_error() {
    static thread_local std::string e;
    return e;
}
bool debug_log() {
    const char *e = std::getenv("NORI_DEBUG");
    return e && e[0] == '1';
}

// rfilter.cpp -> tabulated filter (block.cpp:54-66)
static float filter_eval(const nori_camera_desc &c, float x) {
    switch (c.filter_type) {
    case NORI_FILTER_GAUSSIAN: {
        float alpha = -1.0f / (2.0f * c.filter_p0 * c.filter_p0);
        float v = std::exp(alpha * x * x) - std::exp(alpha * c.filter_radius * c.filter_radius);
        return 0.0f < v ? v : 0.0f;
    }
    case NORI_FILTER_MITCHELL: {
        float B = c.filter_p0, C = c.filter_p1;
        x = std::fabs(2.0f * x / c.filter_radius);
        float x2 = x * x, x3 = x2 * x;
        if (x < 1) return 1.0f / 6.0f * ((12 - 9 * B - 6 * C) * x3 + (-18 + 12 * B + 6 * C) * x2 + (6 - 2 * B));
        if (x < 2) return 1.0f / 6.0f * ((-B - 6 * C) * x3 + (6 * B + 30 * C) * x2 + (-12 * B - 48 * C) * x + (8 * B + 24 * C));
        return 0.0f;
    }
    case NORI_FILTER_TENT: {
        float v = 1.0f - std::fabs(x);
        return 0.0f < v ? v : 0.0f;
    }
    case NORI_FILTER_BOX: return 1.0f;
    case NORI_FILTER_WINDOWED: {
        x = std::fabs(x);
        const float pi = 3.14159265358979323846f;
        auto sinc = [&](float y) { return y < 1e-5f ? 1.0f : std::sin(pi * y) / (pi * y); };
        return sinc(x) * sinc(x / c.filter_p0);
    }
    }
    return 0.0f;
}
int film_border(const nori_camera_desc &c) { return (int)std::ceil(c.filter_radius - 0.5f); }
// k_splat's weights from a jitter class (device_math.h jit_class) need every
// step of ImageBlock::put's index arithmetic exact: a power-of-two radius and
// lookup factor (radius * lookup = NORI_FILTER_RESOLUTION), lookup <= 64 so
// that a class fits 8 bits.  The reference's default radii (gaussian and
// Mitchell 2, tent 1, box 0.5) qualify; other filters keep the pcg32 jitter.
static bool pow2f(float v) {
    int e = 0;
    return v > 0.0f && std::frexp(v, &e) == 0.5f;
}
int jit_code_lookup(float radius, float lookup) {
    if (const char *e = std::getenv("NORI_JIT_CODE"); e && e[0] == '0') return 0;  // A/B
    if (!pow2f(radius) || !pow2f(lookup) || lookup > 64.0f || radius * lookup != (float)NORI_FILTER_RESOLUTION)
        return 0;
    return (int)lookup;
}
void filter_table(const nori_camera_desc &c, float *t) {
    for (int i = 0; i < NORI_FILTER_RESOLUTION; ++i) t[i] = filter_eval(c, (c.filter_radius * i) / NORI_FILTER_RESOLUTION);
    t[NORI_FILTER_RESOLUTION] = 0.0f;
}

// EnvironmentMap tables (envmap.cpp:13-58, 91-109), appended to `env`.
// precompute1D literally: res is the LAST value of `i + f(row, i)`, and the CDF
// accumulates pf(i - 1), a column-major linear index into the whole pf matrix
// (rows not yet computed read as 0, as from a fresh allocation).
static float env_precompute1D(int row, const float *f, int cols, float *pf, float *Pf, int pf_rows) {
    float res = 0;
    int i;
    for (i = 0; i < cols; i++) res = (float)i + f[(size_t)row * cols + i];
    if (res == 0) return res;
    for (int j = 0; j < cols; j++) pf[(size_t)row * cols + j] = f[(size_t)row * cols + j] / res;
    Pf[(size_t)row * (cols + 1)] = 0;
    for (i = 1; i < cols; i++) {
        const int k = i - 1;
        Pf[(size_t)row * (cols + 1) + i] =
            Pf[(size_t)row * (cols + 1) + i - 1] + pf[(size_t)(k % pf_rows) * cols + (k / pf_rows)];
    }
    Pf[(size_t)row * (cols + 1) + i] = 1;
    return res;
}
EnvTables build_envmap(const nori_emitter_desc &e, std::vector<float> &env) {
    const int R = e.env_rows, C = e.env_cols;
    if (R < 2 || C < 2 || !e.env_rgb) throw NoriException(NORI_ERR_INVALID, "EnvMap: the image needs at least 2x2 texels");
    EnvTables o;
    auto grab = [&](size_t n) {
        const size_t off = env.size();
        env.resize(off + n, 0.0f);
        return (uint32_t)off;
    };
    o.rgb_off = grab(3 * (size_t)R * C);
    std::memcpy(&env[o.rgb_off], e.env_rgb, 12 * (size_t)R * C);
    o.pdf_off = grab((size_t)R * C);
    o.cdf_off = grab((size_t)R * (C + 1));
    o.pmarg_off = grab((size_t)R);
    o.cmarg_off = grab((size_t)R + 1);
    if (env.size() >= (1ull << 32)) throw NoriException(NORI_ERR_UNSUPPORTED, "EnvMap: tables above 4G floats");
    std::vector<float> lum((size_t)R * C), sum((size_t)R);
    for (int i = 0; i < R; i++)
        for (int j = 0; j < C; j++) {
            const float *c = e.env_rgb + 3 * ((size_t)i * C + j);
            lum[(size_t)i * C + j] =
                std::sqrt((e.lum_scale[0] * c[0] + e.lum_scale[1] * c[1]) + e.lum_scale[2] * c[2]) + NORI_EPSILON / 10000000;
        }
    for (int i = 0; i < R; ++i) sum[i] = env_precompute1D(i, lum.data(), C, &env[o.pdf_off], &env[o.cdf_off], R);
    env_precompute1D(0, sum.data(), R, &env[o.pmarg_off], &env[o.cmarg_off], 1);
    return o;
}

// BlockGenerator spiral (block.cpp:140-188)
std::vector<uint32_t> spiral_blocks(int W, int H) {
    int nx = (int)std::ceil(W / (float)NORI_BLOCK_SIZE), ny = (int)std::ceil(H / (float)NORI_BLOCK_SIZE);
    std::vector<uint32_t> out;
    int left = nx * ny, dir = 0, bx = nx / 2, by = ny / 2, steps = 1, numSteps = 1;
    while (left > 0) {
        out.push_back((uint32_t)(by * nx + bx));
        if (--left == 0) break;
        do {
            switch (dir) {
            case 0: ++bx; break;
            case 1: ++by; break;
            case 2: --bx; break;
            default: --by; break;
            }
            if (--steps == 0) {
                dir = (dir + 1) % 4;
                if (dir == 2 || dir == 0) ++numSteps;
                steps = numSteps;
            }
        } while (bx < 0 || by < 0 || bx >= nx || by >= ny);
    }
    return out;
}

// Scene box = BVH root box: every mesh vertex and every sphere's bounds.
void scene_root_box(const nori_scene_desc &d, float rmin[3], float rmax[3]) {
    for (int k = 0; k < 3; ++k) rmin[k] = __builtin_inff(), rmax[k] = -__builtin_inff();
    auto expand = [&](float x, float y, float z) {
        float p[3] = {x, y, z};
        for (int k = 0; k < 3; ++k) {
            rmin[k] = std::fmin(rmin[k], p[k]);
            rmax[k] = std::fmax(rmax[k], p[k]);
        }
    };
    for (uint32_t s = 0; s < d.num_shapes; ++s) {
        const nori_shape_desc &sd = d.shapes[s];
        if (sd.type == NORI_SHAPE_SPHERE) {
            expand(sd.center[0] - sd.radius, sd.center[1] - sd.radius, sd.center[2] - sd.radius);
            expand(sd.center[0] + sd.radius, sd.center[1] + sd.radius, sd.center[2] + sd.radius);
        } else {
            for (uint32_t v = 0; v < sd.vtx_count; ++v) {
                const float *p = d.positions + 3 * (size_t)(sd.vtx_offset + v);
                expand(p[0], p[1], p[2]);
            }
        }
    }
}

// DevShape::solitary for every sphere: no other primitive comes within a
// margin of its closed ball and the ball lies inside the scene box (rmin,
// rmax) by that margin.  Closest point of a triangle to the centre: Ericson,
// Real-Time Collision Detection 5.1.5, in double precision.
static double point_triangle_dist2(const double p[3], const float *a, const float *b, const float *c) {
    double ab[3], ac[3], ap[3];
    for (int k = 0; k < 3; ++k) ab[k] = (double)b[k] - a[k], ac[k] = (double)c[k] - a[k], ap[k] = p[k] - a[k];
    auto dot = [](const double *x, const double *y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; };
    auto dist2 = [&](const double q[3]) {
        double s = 0;
        for (int k = 0; k < 3; ++k) s += (p[k] - q[k]) * (p[k] - q[k]);
        return s;
    };
    double q[3];
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0 && d2 <= 0) { for (int k = 0; k < 3; ++k) q[k] = a[k]; return dist2(q); }
    double bp[3];
    for (int k = 0; k < 3; ++k) bp[k] = p[k] - b[k];
    const double d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0 && d4 <= d3) { for (int k = 0; k < 3; ++k) q[k] = b[k]; return dist2(q); }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0 && d1 >= 0 && d3 <= 0) {
        const double v = d1 / (d1 - d3);
        for (int k = 0; k < 3; ++k) q[k] = a[k] + v * ab[k];
        return dist2(q);
    }
    double cp[3];
    for (int k = 0; k < 3; ++k) cp[k] = p[k] - c[k];
    const double d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0 && d5 <= d6) { for (int k = 0; k < 3; ++k) q[k] = c[k]; return dist2(q); }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0 && d2 >= 0 && d6 <= 0) {
        const double w = d2 / (d2 - d6);
        for (int k = 0; k < 3; ++k) q[k] = a[k] + w * ac[k];
        return dist2(q);
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0) {
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        for (int k = 0; k < 3; ++k) q[k] = b[k] + w * ((double)c[k] - b[k]);
        return dist2(q);
    }
    const double den = 1.0 / (va + vb + vc), v = vb * den, w = vc * den;
    for (int k = 0; k < 3; ++k) q[k] = a[k] + ab[k] * v + ac[k] * w;
    return dist2(q);
}

std::vector<uint8_t> solitary_spheres(const nori_scene_desc &d, const float rmin[3], const float rmax[3]) {
    std::vector<uint8_t> solitary(d.num_shapes, 0);
    if (const char *e = std::getenv("NORI_CHORD"); e && e[0] == '0') return solitary;  // A/B: full scans only
    for (uint32_t s = 0; s < d.num_shapes; ++s) {
        const nori_shape_desc &sp = d.shapes[s];
        if (sp.type != NORI_SHAPE_SPHERE || !(sp.radius > 0.0f)) continue;
        const double r = sp.radius, c[3] = {sp.center[0], sp.center[1], sp.center[2]};
        const double margin = 1e-4 * (std::max({std::fabs(c[0]), std::fabs(c[1]), std::fabs(c[2])}) + r);
        bool ok = true;
        for (int k = 0; k < 3 && ok; ++k) ok = c[k] - r > (double)rmin[k] + margin && c[k] + r < (double)rmax[k] - margin;
        const double reach = r + margin;
        for (uint32_t o = 0; o < d.num_shapes && ok; ++o) {
            if (o == s) continue;
            const nori_shape_desc &od = d.shapes[o];
            if (od.type == NORI_SHAPE_SPHERE) {
                double dd = 0;
                for (int k = 0; k < 3; ++k) dd += (c[k] - od.center[k]) * (c[k] - od.center[k]);
                ok = std::sqrt(dd) > reach + od.radius;
                continue;
            }
            for (uint32_t t = 0; t < od.tri_count && ok; ++t) {
                const uint32_t *f = d.indices + 3 * (size_t)(od.tri_offset + t);
                const float *p0 = d.positions + 3 * (size_t)f[0], *p1 = d.positions + 3 * (size_t)f[1],
                            *p2 = d.positions + 3 * (size_t)f[2];
                bool far = false;  // quick reject: the triangle's box misses the ball's box
                for (int k = 0; k < 3; ++k)
                    far = far || std::min({p0[k], p1[k], p2[k]}) > c[k] + reach || std::max({p0[k], p1[k], p2[k]}) < c[k] - reach;
                if (!far) ok = point_triangle_dist2(c, p0, p1, p2) > reach * reach;
            }
        }
        solitary[s] = ok ? 1 : 0;
        if (std::getenv("NORI_DEBUG")) std::fprintf(stderr, "[nori] sphere shape %u: solitary %d\n", s, (int)ok);
    }
    return solitary;
}

// The in-plane filter of the binned extension kernel (scan.h
// pair_candidate): a ray can be accepted by the Moller-Trumbore test of a
// triangle of pair g only if its crossing with the pair's plane x_A = c lies
// within the pair's in-plane bounding rectangle widened by a margin M that
// covers every rounding error of the test.  Derivation (A the plane axis, B
// and C the other two, u = 2^-24, gamma_k = k u / (1 - k u)): with e1_A =
// e2_A = 0, the reference's u numerator tvec . (d x e2) divided by the exact
// det = -d_A n (n = e1_B e2_C - e1_C e2_B) is a sum of terms bounded by
// E (|o_B - v0_B| + |o_C - v0_C| + |t*| (|d_B| + |d_C|)) / |n| = E L / |n|
// (E the largest in-plane edge component, t* = (c - o_A) / d_A the exact
// crossing), each computed with at most 6 roundings, and det carries
// (2 kappa + 1) u (kappa <= 32, axis_plane); so the computed u and v differ
// from the exact barycentrics of the crossing by at most
// gamma_8 E L / |n| + gamma_(2 kappa + 6) each.  An accepted (u, v) lies in
// the triangle (u + v <= 1 up to one rounding), hence the exact crossing lies
// within 2 E (gamma_8 E L / |n| + gamma_(2 kappa + 6)) + 2^-23 E of the
// triangle's bounding box in B and C.  The kernel computes the crossing as
// t_f = (c - o_A) * (1 / d_A) (3 roundings of t*) and d_B = o_B + t_f d_B -
// mid_B, whose own error is below gamma_8 S + 2^-22 |mid_B| with
// S = |o_B| + |o_C| + |t_f| (|d_B| + |d_C|) >= L - V, V = |v0_B| + |v0_C|.
// Hence the test  |d_B| <= half_B + Ka S + Kb  (and the same in C) with
//     Ka = (2 gamma_8 E^2 / n_min + gamma_8) * 1.05
//     Kb = (2 gamma_8 E^2 / n_min * V + 2 E gamma_70 + 2^-23 E + 2^-22 |mid|) * 1.05
// never rejects an accepted ray (the factor 1.05 covers the roundings of the
// filter's own products).  Per pair: (mid_B, half_B + Kb, mid_C, half_C + Kb),
// (Ka, c, 0, 0).  A padding record (zero edges) never hits and is left out.
static void plane_filters(ScanList &L) {
    const uint32_t npairs = (uint32_t)L.plane_c.size();
    L.plane_f.assign(8 * (size_t)npairs, 0.0f);
    const double u = std::ldexp(1.0, -24);
    auto gam = [&](double k) { return k * u / (1.0 - k * u); };
    auto up = [](double x) {  // the float >= x
        float f = (float)x;
        return (double)f < x ? std::nextafter(f, INFINITY) : f;
    };
    for (uint32_t g = 0; g < npairs; ++g) {
        const int A = g < L.plane_end[0] ? 0 : g < L.plane_end[1] ? 1 : 2, B = (A + 1) % 3, C = (A + 2) % 3;
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        double E = 0.0, nmin = INFINITY, V = 0.0;
        for (int k = 0; k < 2; ++k) {
            const float *r = &L.prims[12 * (size_t)(2 * g + k)];
            const float *v0 = r, *e1 = r + 4, *e2 = r + 8;
            const double n = std::fabs((double)e1[B] * e2[C] - (double)e1[C] * e2[B]);
            if (n == 0.0) continue;  // padding record
            for (int a : {B, C}) {
                for (double x : {(double)v0[a], (double)v0[a] + e1[a], (double)v0[a] + e2[a]}) {
                    lo[a] = std::min(lo[a], x);
                    hi[a] = std::max(hi[a], x);
                }
                E = std::max({E, std::fabs((double)e1[a]), std::fabs((double)e2[a])});
            }
            nmin = std::min(nmin, n);
            V = std::max(V, std::fabs((double)v0[B]) + std::fabs((double)v0[C]));
        }
        float *f = &L.plane_f[8 * (size_t)g];
        if (!(nmin < INFINITY)) {  // two padding records: an empty rectangle no ray passes
            f[0] = f[2] = 0.0f;
            f[1] = f[3] = -1.0f;
            f[5] = L.plane_c[g];
            continue;
        }
        const double K1 = 2.0 * gam(8) * E * E / nmin;
        const double Ka = (K1 + gam(8)) * 1.05;
        for (int k = 0; k < 2; ++k) {
            const int a = k ? C : B;
            const float mid = (float)(0.5 * (lo[a] + hi[a]));
            const double half = std::max(hi[a] - mid, mid - lo[a]);
            const double Kb = (K1 * V + 2.0 * E * gam(70) + std::ldexp(E, -23) + std::ldexp(std::fabs(mid), -22)) * 1.05;
            f[2 * k] = mid;
            f[2 * k + 1] = (float)up(up(half) + Kb);
        }
        f[4] = (float)up(Ka);
        f[5] = L.plane_c[g];
    }
}
static bool axis_plane(const float *r, int a) {
    const float *e1 = r + 4, *e2 = r + 8;
    if (e1[a] != 0.0f || e2[a] != 0.0f) return false;
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    for (int k : {b, c}) {  // products of normal range: nonzero components in [2^-60, 2^60]
        for (float x : {e1[k], e2[k]})
            if (x != 0.0f && !(std::fabs(x) >= 0x1p-60f && std::fabs(x) <= 0x1p60f)) return false;
    }
    // det and t's numerator are (ray component) x (P - Q) with P, Q the two
    // products below: kappa = (|P| + |Q|) / |P - Q| bounds their rounding
    const double P = (double)e1[b] * e2[c], Q = (double)e1[c] * e2[b];
    const double diff = std::fabs(P - Q);
    return diff > 0.0 && (std::fabs(P) + std::fabs(Q)) <= 32.0 * diff;
}
static ScanList build_scan_list_(const DeviceBvh &bvh, uint32_t n);
float scan_fast_max(const ScanList &L) {
    if (const char *e = std::getenv("NORI_SCAN_FAST"); e && e[0] == '0') return 0.0f;
    // E: the largest edge component, V: the largest v0 component of the triangle records
    double E = 0.0, V = 0.0;
    for (uint32_t i = 0; i < L.tris; ++i) {
        const float *r = &L.prims[12 * (size_t)i];
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(r[k]) || !std::isfinite(r[4 + k]) || !std::isfinite(r[8 + k])) return 0.0f;
            V = std::max(V, std::fabs((double)r[k]));
            E = std::max({E, std::fabs((double)r[4 + k]), std::fabs((double)r[8 + k])});
        }
    }
    // |o_i|, |d_i| <= M.  In magnitude, per component: tvec = o - v0 <= M + V;
    // pvec = d x e2 <= 2 M E; qvec = tvec x e1 <= 2 (M + V) E; and the dots
    // det = e1 . pvec, tvec . pvec, d . qvec, e2 . qvec three such products
    // each; d . d <= 3 M^2.  Every partial sum obeys the same bound, and the
    // roundings of at most five operations are inside the factor `slack`.
    const double lim = std::ldexp(1.0, 125), slack = 1.0 + std::ldexp(1.0, -20);
    auto fits = [&](double M) {
        const double tv = M + V, pv = 2.0 * M * E, qv = 2.0 * tv * E;
        const double worst = std::max({tv, pv, qv, 3.0 * E * pv, 3.0 * tv * pv, 3.0 * M * qv, 3.0 * E * qv, 6.0 * M * M});
        return worst * slack <= lim;
    };
    double M = std::ldexp(1.0, 60);
    while (M >= 1.0 && !fits(M)) M *= 0.5;
    if (M < 1.0 || M < 16.0 * std::max(V, E)) return 0.0f;
    return (float)M;
}
ScanList build_scan_list(const DeviceBvh &bvh, uint32_t n) {
    ScanList L = build_scan_list_(bvh, n);
    L.fast_max = scan_fast_max(L);
    return L;
}
static ScanList build_scan_list_(const DeviceBvh &bvh, uint32_t n) {
    ScanList L;
    auto rec = [&](uint32_t i) { return &bvh.prims[12 * (size_t)i]; };
    auto sphere = [&](uint32_t i) {
        uint32_t f;
        std::memcpy(&f, rec(i) + 7, 4);
        return f != 0u;
    };
    auto add = [&](uint32_t i) {
        const float *r = rec(i);
        L.prims.insert(L.prims.end(), r, r + 12);
        std::memcpy(&L.prims[L.prims.size() - 1], &i, 4);  // e2.w = leaf-order position
    };
    auto add_null = [&] {
        float null_prim[12] = {0};  // zero edges: det = 0, never hit
        const uint32_t none = 0xFFFFFFFFu;
        std::memcpy(&null_prim[3], &none, 4);
        L.prims.insert(L.prims.end(), null_prim, null_prim + 12);
    };
    if (const char *e = std::getenv("NORI_PLANE_CULL"); e && e[0] == '0') {  // A/B: no plane pairs
        for (uint32_t i = 0; i < n; ++i)
            if (!sphere(i)) add(i), ++L.tris;
        L.real = L.tris;
        for (; L.tris % kScanListGroup; ++L.tris) add_null();
        for (uint32_t i = 0; i < n; ++i)
            if (sphere(i)) add(i);
        return L;
    }
    std::vector<int> axis(n, -1);
    for (uint32_t i = 0; i < n; ++i)
        if (!sphere(i))
            for (int a = 0; a < 3 && axis[i] < 0; ++a)
                if (axis_plane(rec(i), a)) axis[i] = a;
    for (int a = 0; a < 3; ++a) {
        // this axis's planes in order of first appearance (leaf order)
        std::vector<float> planes;
        for (uint32_t i = 0; i < n; ++i)
            if (axis[i] == a && std::find(planes.begin(), planes.end(), rec(i)[a]) == planes.end())
                planes.push_back(rec(i)[a]);
        for (float c : planes) {
            uint32_t in_pair = 0;
            for (uint32_t i = 0; i < n; ++i)
                if (axis[i] == a && rec(i)[a] == c) {
                    add(i);
                    if (++in_pair == 2) {
                        L.plane_c.push_back(c);
                        in_pair = 0;
                    }
                }
            if (in_pair) {
                add_null();
                L.plane_c.push_back(c);
            }
        }
        L.plane_end[a] = (uint32_t)L.plane_c.size();
    }
    L.tris = 2 * (uint32_t)L.plane_c.size();
    uint32_t rest = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (!sphere(i) && axis[i] < 0) add(i), ++rest;
    L.real = L.tris + rest;
    for (; rest % kScanListGroup; ++rest) add_null();
    L.tris += rest;
    for (uint32_t i = 0; i < n; ++i)
        if (sphere(i)) add(i);
    plane_filters(L);
    if (debug_log())
        std::fprintf(stderr, "[nori] scan list: %zu axis-plane pairs (x %u, y %u, z %u), %u other triangle records\n",
                     L.plane_c.size(), L.plane_end[0], L.plane_end[1] - L.plane_end[0],
                     L.plane_end[2] - L.plane_end[1], rest);
    return L;
}

bool basic_scene(const nori_scene_desc &d) {
    if (const char *e = std::getenv("NORI_BASIC"); e && e[0] == '0') return false;
    for (uint32_t i = 0; i < d.num_bsdfs; ++i) {
        const nori_bsdf_desc &b = d.bsdfs[i];
        if (b.type != NORI_BSDF_DIFFUSE && b.type != NORI_BSDF_MIRROR && b.type != NORI_BSDF_DIELECTRIC) return false;
        if (b.type == NORI_BSDF_DIFFUSE && b.albedo_texture != NORI_TEXTURE_CONSTANT) return false;
    }
    for (uint32_t i = 0; i < d.num_emitters; ++i)
        if (d.emitters[i].type != NORI_EMITTER_AREA) return false;
    for (uint32_t i = 0; i < d.num_shapes; ++i)
        if (d.shapes[i].normal_map >= 0) return false;
    return d.camera.camera_type == NORI_CAMERA_PERSPECTIVE;
}

}  // namespace nori

using namespace nori;

extern "C" {

const char *nori_gpu_last_error(void) { return last_error().c_str(); }
int nori_gpu_abi_version(void) { return NORI_GPU_ABI_VERSION; }

int nori_read_image(const char *path, int *width, int *height, uint8_t *rgb) {
    return guarded([&] {
        if (!path || !width || !height) return fail(NORI_ERR_INVALID, "null argument");
        int w = 0, h = 0;
        std::vector<uint8_t> img;
        decode_image_rgb8(path, w, h, img);
        *width = w;
        *height = h;
        if (rgb) std::memcpy(rgb, img.data(), img.size());
        return NORI_OK;
    });
}

int nori_scene_load_xml(const char *path, int width, int height, int spp, nori_scene **out) {
    return guarded([&] {
        if (!path || !out) return fail(NORI_ERR_INVALID, "null argument");
        auto *s = new nori_scene;
        s->hs.reset(load_scene_xml(path, width, height, spp));
        *out = s;
        return NORI_OK;
    });
}
const nori_scene_desc *nori_scene_get_desc(const nori_scene *s) { return s ? &s->hs->desc : nullptr; }

void nori_scene_free(nori_scene *s) { delete s; }

int nori_film_border(const nori_scene_desc *d) { return d ? film_border(d->camera) : NORI_ERR_INVALID; }
int nori_filter_table(const nori_scene_desc *d, float *table) {
    if (!d || !table) return fail(NORI_ERR_INVALID, "null argument");
    filter_table(d->camera, table);
    return NORI_OK;
}
int nori_film_develop(const nori_scene_desc *d, const float *rgbw, float *rgb) {
    if (!d || !rgbw || !rgb) return fail(NORI_ERR_INVALID, "null argument");
    int W = d->camera.width, H = d->camera.height, B = film_border(d->camera), FW = W + 2 * B;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const float *c = rgbw + 4 * ((size_t)(y + B) * FW + (x + B));
            float *o = rgb + 3 * ((size_t)y * W + x);
            for (int k = 0; k < 3; ++k) o[k] = c[3] != 0 ? c[k] / c[3] : 0.0f;  // color.h:113-118
        }
    return NORI_OK;
}

int nori_scene_bvh_rebuild(const nori_scene_desc *d, const float *positions, uint32_t leaf_max,
                           const float *refit_positions, nori_bvh_rebuild_info *info, float *nodes, float *prims,
                           float *root_box) {
    return guarded([&] {
        if (!d) return fail(NORI_ERR_INVALID, "null argument");
        if (d->abi_version != NORI_GPU_ABI_VERSION) return fail(NORI_ERR_INVALID, "ABI version mismatch");
        if (leaf_max > kRebuildLeafMax) return fail(NORI_ERR_INVALID, "nori_scene_bvh_rebuild: leaf_max above 64");
        for (const float *p : {positions, refit_positions})
            if (p)
                for (size_t i = 0; i < 3 * (size_t)d->num_vertices; ++i)
                    if (!std::isfinite(p[i])) return fail(NORI_ERR_INVALID, "nori_scene_bvh_rebuild: a non-finite position");
        DeviceBvh bvh;
        rebuild_host(*d, positions, leaf_max, bvh);
        if (refit_positions) refit_host(bvh, build_refit_plan(bvh), prim_vertex_ids(*d), refit_positions, nullptr);
        if (info) {
            std::memset(info, 0, sizeof(*info));
            info->device_nodes = bvh.num_nodes;
            info->depth = bvh.depth;
            info->num_prims = (uint32_t)(bvh.prims.size() / 12);
            info->leaf_max = leaf_max ? leaf_max : kRebuildLeafDefault;
        }
        if (nodes) std::memcpy(nodes, bvh.nodes.data(), bvh.nodes.size() * 4);
        if (prims) std::memcpy(prims, bvh.prims.data(), bvh.prims.size() * 4);
        if (root_box) refit_root_box(bvh.nodes.data(), root_box);
        return NORI_OK;
    });
}

}  // extern "C"
