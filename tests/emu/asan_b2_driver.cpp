// tests/emu/asan_b2_driver.cpp -- qpx_backward2 (the second-order pass of the backward) on the host-thread
// emulation under AddressSanitizer + UBSan.  TEST INFRASTRUCTURE ONLY.  Every array has exactly the size the C ABI documents and
// the emulated LDS exactly the size the launcher asks for (QPX_EMU_LDS_SLACK = 0), so an index one element out of range --
// silent on the GPU -- is a reported overflow.  Usage: asan_b2_driver <B> <n> <m> <q> [variant [wide]]; exit code 0 = clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/qpx.h"

static double urand(unsigned& s)
{
    s = s * 1664525u + 1013904223u;
    return (double)(s >> 8) / (double)(1u << 24);
}

template <class T> static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

// the whole sequence in element type T (double: QPX_F64, float: QPX_F32_WIDE), from float64 problem data
template <class T>
static int run(int dtype, int B, int n, int m, int q, const std::vector<double>& Qd, const std::vector<double>& pd,
               const std::vector<double>& Gd, const std::vector<double>& hd, const std::vector<double>& Ad, const std::vector<double>& bd)
{
    auto cast = [](const std::vector<double>& v) { return std::vector<T>(v.begin(), v.end()); };
    std::vector<T> Q = cast(Qd), p = cast(pd), G = cast(Gd), h = cast(hd), A = cast(Ad), bb = cast(bd);
    const size_t fe = qpx_factor_elems(dtype, n, m, q);
    std::vector<double> fac((size_t)B * fe);            // (QPX_F32_WIDE: the blob holds doubles)
    std::vector<T> zhat((size_t)B * n), nu((size_t)B * q), lam((size_t)B * m), sl((size_t)B * m), br(B);
    std::vector<int32_t> status(B), iters(B);
    int rc = qpx_forward(dtype, B, n, m, q, Q.data(), (int64_t)n * n, p.data(), n, G.data(), (int64_t)m * n, h.data(), m, ptr(A),
                         (int64_t)q * n, ptr(bb), q, fac.data(), 1e-12, 20, 3, B == 1 ? 1 : 2, zhat.data(), ptr(nu), lam.data(),
                         sl.data(), iters.data(), status.data(), br.data(), nullptr, nullptr);
    if (rc) { fprintf(stderr, "forward rc %d\n", rc); return 2; }
    std::vector<T> g((size_t)B * n, T(1)), dx((size_t)B * n), dz((size_t)B * m), dy((size_t)B * q);
    rc = qpx_backward(dtype, B, n, m, q, fac.data(), (int64_t)fe, zhat.data(), lam.data(), sl.data(), ptr(nu), g.data(), nullptr,
                      nullptr, nullptr, nullptr, nullptr, nullptr, dx.data(), dz.data(), ptr(dy), 0, nullptr, 0, nullptr, 0,
                      nullptr, 0, status.data(), nullptr);
    if (rc) { fprintf(stderr, "backward rc %d\n", rc); return 2; }
    if (!qpx_backward2_supported(dtype, n, m, q)) { fprintf(stderr, "qpx_backward2 not served at this size / knob\n"); return 4; }
    unsigned seed = 777;
    auto rnd = [&](size_t cnt) { std::vector<T> v(cnt); for (auto& x : v) x = (T)(urand(seed) - 0.5); return v; };
    std::vector<T> WQ = rnd((size_t)n * n) /* shared: stride 0 */, Wp = rnd((size_t)B * n), WG = rnd((size_t)B * m * n), Wh = rnd((size_t)m) /* shared */;
    std::vector<T> WA = rnd((size_t)B * q * n), Wb = rnd((size_t)B * q);
    std::vector<T> zd((size_t)B * n), ld((size_t)B * m), nd((size_t)B * q), HQ((size_t)B * n * n), Hp((size_t)B * n), HG((size_t)B * m * n);
    std::vector<T> Hh((size_t)B * m), HA((size_t)B * q * n), Hb((size_t)B * q);
    rc = qpx_backward2(dtype, B, n, m, q, fac.data(), (int64_t)fe, zhat.data(), lam.data(), sl.data(), ptr(nu), dx.data(), dz.data(), ptr(dy),
                       WQ.data(), 0, Wp.data(), n, WG.data(), (int64_t)m * n, Wh.data(), 0, ptr(WA), (int64_t)q * n, ptr(Wb), q,
                       zd.data(), ld.data(), ptr(nd), HQ.data(), Hp.data(), HG.data(), Hh.data(), ptr(HA), ptr(Hb), status.data(), nullptr);
    if (rc) { fprintf(stderr, "backward2 rc %d\n", rc); return 2; }
    // ... and with every optional argument NULL
    std::vector<T> zd2((size_t)B * n);
    rc = qpx_backward2(dtype, B, n, m, q, fac.data(), (int64_t)fe, zhat.data(), lam.data(), sl.data(), ptr(nu), dx.data(), dz.data(), ptr(dy),
                       nullptr, 0, Wp.data(), n, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0,
                       zd2.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, status.data(), nullptr);
    if (rc) { fprintf(stderr, "backward2 (NULLs) rc %d\n", rc); return 2; }
    double worst = 0;
    for (const auto* v : {&zd, &ld, &HQ, &Hp, &HG, &Hh, &zd2})
        for (T x : *v) { if (!(x == x)) { fprintf(stderr, "backward2: NaN in an output\n"); return 3; } worst = std::fmax(worst, std::fabs((double)x)); }
    for (int s = 0; s < B; ++s)
        if (status[s] & QPX_ST_KKT_BREAKDOWN) { fprintf(stderr, "backward2: breakdown in qp %d\n", s); return 5; }
    printf("dtype %d: max |output| %.3e\n", dtype, worst);
    return worst > 0 ? 0 : 6;
}

int main(int argc, char** argv)
{
    const int B = argc > 1 ? atoi(argv[1]) : 1, n = argc > 2 ? atoi(argv[2]) : 12, m = argc > 3 ? atoi(argv[3]) : 9;
    const int q = argc > 4 ? atoi(argv[4]) : 3;
    if (argc > 5) qpx_set_ipm_variant(atoi(argv[5]));
    unsigned seed = 12345;
    std::vector<double> Q((size_t)B * n * n), p((size_t)B * n), G((size_t)B * m * n), h((size_t)B * m), A((size_t)B * q * n), bb((size_t)B * q);
    for (int s = 0; s < B; ++s) {
        std::vector<double> L((size_t)n * n), z0(n);
        for (auto& v : L) v = urand(seed) - 0.5;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                double acc = (i == j) ? 1e-3 : 0.0;
                for (int k = 0; k < n; ++k) acc += L[(size_t)i * n + k] * L[(size_t)j * n + k];
                Q[((size_t)s * n + i) * n + j] = acc;
            }
        for (int i = 0; i < n; ++i) { p[(size_t)s * n + i] = urand(seed) - 0.5; z0[i] = urand(seed) - 0.5; }
        for (int i = 0; i < m; ++i) {
            double acc = 0;
            for (int j = 0; j < n; ++j) { const double g = urand(seed) - 0.5; G[((size_t)s * m + i) * n + j] = g; acc += g * z0[j]; }
            h[(size_t)s * m + i] = acc + urand(seed);                 // feasible: h = G z0 + s0, s0 > 0
        }
        for (int i = 0; i < q; ++i) {
            double acc = 0;
            for (int j = 0; j < n; ++j) { const double a = urand(seed) - 0.5; A[((size_t)s * q + i) * n + j] = a; acc += a * z0[j]; }
            bb[(size_t)s * q + i] = acc;
        }
    }
    int rc = run<double>(QPX_F64, B, n, m, q, Q, p, G, h, A, bb);
    if (rc) return rc;
    if (argc > 6 && std::string(argv[6]) == "wide") return run<float>(QPX_F32_WIDE, B, n, m, q, Q, p, G, h, A, bb);
    return 0;
}
