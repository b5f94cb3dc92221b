// dispatch_trace.cpp -- prints, for a sweep of (entry point, dtype, B, n, m, q, knob), every launch the dispatcher of
// qpx_api.inc would make: launcher + template arguments, batch, LDS bytes, and for the large-QP family a hash of the
// argument struct.  No kernel body runs.  Build (from the repository root):
//   g++ -O1 -std=c++17 -w -Itests/emu -Iqpth_amd/csrc -o dispatch_trace scripts/dispatch_trace.cpp
// Compare the output (or its sha256) between two trees.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/qpx.h"
#include "qpx_platform.h"
#include "qpx_kernels.h"
#include "qpx_grid.h"
#include "qpx_tile.h"
#include "qpx_prefac.h"
#include "qpx_reduce.h"
#include "qpx_big.h"
#include "qpx_big_polish.h"

namespace qpx {
template <int V> using Int = std::integral_constant<int, V>;
template <bool V> using Bool = std::integral_constant<bool, V>;
inline size_t lds_budget_bytes() { return kMaxLdsBytes; }
void fiber_wait(FiberSched*, FiberBar*, int) {}

static const char* tn(float) { return "f32"; }
static const char* tn(double) { return "f64"; }
template <class A> static unsigned long long hashof(const A& a)
{
    unsigned long long h = 1469598103934665603ull;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(&a);
    for (size_t i = 0; i < sizeof(A); ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}
#define OUT(...) (std::printf(__VA_ARGS__), std::printf("\n"), QPX_OK)

template <class T, int NBL> int launch_sweep(const PrefactorArgs<T>& a, size_t l, void*) { return OUT("  sweep<%s,%d> B=%d images=%d lds=%zu", tn(T()), NBL, a.B, a.images, l); }
template <int NBN, bool kEq> int launch_prefac_tile(const PrefactorArgs<double>& a, size_t l, void*) { return OUT("  prefac_tile<%d,%d> B=%d images=%d pf=%d,%d lds=%zu", NBN, (int)kEq, a.B, a.images, (int)sizeof(a.pf_k), (int)sizeof(a.pf_r), l); }
template <class T, int NBL, int NS> int launch_ipm_grid(const IpmArgs<T>& a, size_t l, void*) { return OUT("  ipm_grid16<%s,%d,%d> B=%d images=%d lds=%zu", tn(T()), NBL, NS, a.B, a.images, l); }
template <class T, int NBL, int NS> int launch_ipm_grid8(const IpmArgs<T>& a, size_t l, void*) { return OUT("  ipm_grid8<%s,%d,%d> B=%d images=%d lds=%zu", tn(T()), NBL, NS, a.B, a.images, l); }
template <int NBL, int NW, int NS, bool CH = false> int launch_ipm_tile(const IpmArgs<double>& a, size_t l, void*) { return OUT("  ipm_tile<%d,%d,%d,%d> B=%d images=%d lds=%zu", NBL, NW, NS, (int)CH, a.B, a.images, l); }
template <int NBL, int NW, bool kBw, bool CH = false> int launch_kkt_tile(const KktArgs<double>& a, size_t l, void*) { return OUT("  kkt_tile<%d,%d,%d,%d> B=%d images=%d jvp=%d lds=%zu", NBL, NW, (int)kBw, (int)CH, a.B, a.images, a.jvp, l); }
template <class T, int NBL, bool kBw> int launch_kkt_grid(const KktArgs<T>& a, size_t l, void*) { return OUT("  kkt_grid<%s,%d,%d> B=%d images=%d jvp=%d lds=%zu", tn(T()), NBL, (int)kBw, a.B, a.images, a.jvp, l); }
template <class T, int NBL> int launch_polish_grid(const PolishArgs<T>& a, size_t l, void*) { return OUT("  polish_grid<%s,%d> B=%d images=%d lds=%zu", tn(T()), NBL, a.B, a.images, l); }
template <int NBL, int NW, bool CH> int launch_polish_tile(const PolishArgs<double>& a, size_t l, void*) { return OUT("  polish_tile<%d,%d,%d> B=%d images=%d lds=%zu", NBL, NW, (int)CH, a.B, a.images, l); }
template <class T> int launch_batch_outer(const OuterArgs<T>& a, int tiles, void*) { return OUT("  batch_outer<%s> B=%d r=%d c=%d tiles=%d chunks=%d chunk_len=%d ws=%d", tn(T()), a.B, a.r, a.c, tiles, a.chunks, a.chunk_len, a.ws != nullptr); }
template <class T> int launch_dense_solve(const DenseSolveArgs<T>& a, void*) { return OUT("  dense_solve<%s> B=%d k=%d", tn(T()), a.B, a.k); }
#define BIG(NAME, ARGS) template <class T> int launch_big_##NAME(const ARGS<T>& a, void* s) { return OUT("  big_" #NAME "<%s> s=%p %016llx", tn(T()), s, hashof(a)); }
#define BIGY(NAME, ARGS) template <class T> int launch_big_##NAME(const ARGS<T>& a, int gy, void* s) { return OUT("  big_" #NAME "<%s> gy=%d s=%p %016llx", tn(T()), gy, s, hashof(a)); }
BIGY(pack, BigPackArgs) BIG(panel, BigPanelArgs) BIG(gemm, BigGemmArgs) BIG(trsv, BigTrsvArgs) BIG(gemv, BigGemvArgs) BIG(symv, BigSymvArgs)
BIG(vec, BigVecArgs) BIGY(kkt, BigKktArgs) BIG(phase, BigPhaseArgs) BIG(solve, BigSolveArgs) BIG(diag, BigDiagArgs) BIG(polish, BigPolishArgs)

int stream_fork(void* caller, int nside, void** side, int delay_us, int first = 0)
{
    for (int i = 0; i < nside; ++i) side[i] = (void*)(uintptr_t)(0x5000 + 16 * (first + i));
    return OUT("  fork caller=%p nside=%d delay=%d first=%d", caller, nside, delay_us, first);
}
int stream_join(void* caller, int nside, void* const* side, int first = 0) { return OUT("  join caller=%p nside=%d side0=%p first=%d", caller, nside, side[0], first); }
}  // namespace qpx

#include "qpx_api.inc"

// fake, never dereferenced, distinct and far apart
static void* P(int i) { return (void*)(uintptr_t)(0x100000000000ull + (uintptr_t)i * 0x4000000000ull); }

static void one(int dt, int B, int n, int m, int q, int knob)
{
    qpx_set_ipm_variant(knob);
    void* st = (void*)(uintptr_t)0x4000;
    const int64_t fe = (int64_t)qpx_factor_elems(dt, n, m, q);
    std::printf("# dt=%d B=%d n=%d m=%d q=%d knob=%d: supported=%d family=%d elems=%lld share=%d refine=%d polish=%d\n", dt, B, n, m, q, knob,
                qpx_supported(dt, n, m, q), qpx_kernel_family(dt, n, m, q), (long long)fe, qpx_can_share_factors(dt, n, m, q),
                qpx_refine_supported(dt, n, m, q), qpx_polish_supported(dt, n, m, q));
    int e;
    e = qpx_pre_factor(dt, B, n, m, q, P(1), (int64_t)n * n, P(2), (int64_t)m * n, P(3), (int64_t)q * n, P(4), (int32_t*)P(5), st);
    std::printf(" pre_factor -> %d\n", e);
    e = qpx_ipm(dt, B, n, m, q, P(6), n, P(7), m, P(8), q, P(4), fe, 1e-12, 2, 3, 2, P(9), P(10), P(11), P(12), (int32_t*)P(13), (int32_t*)P(5), P(14), nullptr, st);
    std::printf(" ipm -> %d\n", e);
    e = qpx_factor_solve_kkt(dt, B, n, m, q, P(4), fe, P(15), P(16), P(17), P(18), P(19), P(20), P(21), P(22), P(23), 0, P(1), (int64_t)n * n, P(2), (int64_t)m * n, P(3), (int64_t)q * n, (int32_t*)P(5), st);
    std::printf(" factor_solve_kkt -> %d\n", e);
    e = qpx_backward(dt, B, n, m, q, P(4), fe, P(9), P(11), P(12), P(10), P(24), P(25), P(26), P(27), P(28), P(29), P(30), P(20), P(22), P(23), 0, P(1), (int64_t)n * n, P(2), (int64_t)m * n, P(3), (int64_t)q * n, (int32_t*)P(5), st);
    std::printf(" backward -> %d\n", e);
    e = qpx_jvp(dt, B, n, m, q, P(4), fe, P(9), P(11), P(12), P(10), P(31), (int64_t)n * n, P(32), n, P(33), (int64_t)m * n, P(34), m, P(35), (int64_t)q * n, P(36), q, P(37), P(38), P(39), P(40), 0, P(1), (int64_t)n * n, P(2), (int64_t)m * n, P(3), (int64_t)q * n, (int32_t*)P(5), st);
    std::printf(" jvp -> %d\n", e);
    // the warm entry and the range / elastic roles of the loop forms (their LDS bytes carry the role's vectors)
    std::printf("# warm=%d range=%d elastic=%d\n", qpx_warm_supported(dt, n, m, q), qpx_range_supported(dt, n, m, q), qpx_elastic_supported(dt, n, m, q));
    e = qpx_ipm_warm(dt, B, n, m, q, P(6), n, P(7), m, P(8), q, P(4), fe, 1e-12, 2, 3, 2, P(9), P(10), P(11), P(12), (int32_t*)P(13), (int32_t*)P(5), P(14), nullptr, P(41), P(42), 1e-2, (int32_t*)P(43), st);
    std::printf(" ipm_warm -> %d\n", e);
    e = qpx_ipm_range(dt, B, n, m, q, P(6), n, P(7), m, P(8), q, P(4), fe, 1e-12, 2, 3, 2, P(9), P(10), P(11), P(12), (int32_t*)P(13), (int32_t*)P(5), P(14), nullptr, P(44), m, P(45), P(46), P(47), st);
    std::printf(" ipm_range -> %d\n", e);
    e = qpx_ipm_elastic(dt, B, n, m, q, P(6), n, P(7), m, P(8), q, P(4), fe, 1e-12, 2, 3, 2, P(9), P(10), P(11), P(12), (int32_t*)P(13), (int32_t*)P(5), P(14), nullptr, P(44), m, P(48), m, P(45), P(46), P(47), P(49), st);
    std::printf(" ipm_elastic -> %d\n", e);
    e = qpx_polish(dt, B, n, m, q, P(1), (int64_t)n * n, P(6), n, P(2), (int64_t)m * n, P(7), m, P(3), (int64_t)q * n, P(8), q, P(4), fe, 2, 0, P(9), P(10), P(11), P(12), P(14), (int32_t*)P(5), st);
    std::printf(" polish -> %d\n", e);
    qpx_set_ipm_variant(0);
}

int main()
{
    const int sizes[] = {1, 2, 5, 8, 16, 17, 32, 33, 48, 64, 65, 80, 100, 112, 113, 128, 130, 150, 180, 200, 208, 300, 513, 1024, 1025};
    const int qs[] = {0, 3, 10, 40};
    const int Bs[] = {1, 8, 95, 96, 512, 513, 1024, 1025, 8192, 8193, 65536};
    const int knobs[] = {0, 3, 256, 512, 1024 + 2048, 1024 + 4096, 1024 + 8192, 1 << 14, (3 << 16) | 3, (1 << 26) | 3, (1 << 27) | 3, (1 << 28) | 3, (1 << 29) | 3};
    for (int dt = 0; dt < 3; ++dt)
        for (int knob : knobs)
            for (int n : sizes)
                for (int m : sizes)
                    for (int q : qs) {
                        const bool big = n + m + q > 208 || (knob & 255) == 3;
                        // the large-QP family makes hundreds of launches per call: a thinner sweep there
                        if (big && ((n != 5 && n != 100 && n != 150 && n != 513 && n != 1024) || (m != 8 && m != 100 && m != 150 && m != 300 && m != 1025) || q == 3 || q == 40)) continue;
                        if ((knob & 255) == 3 && (n > 150 || m > 150)) continue;        // the forced large-QP knob: small sizes are the point
                        for (int B : Bs) {
                            // keep the sweep small: the batch size only matters near the dispatcher's thresholds
                            if (big && B != 1 && B != 95 && B != 96 && B != 512) continue;
                            one(dt, B, n, m, q, knob);
                        }
                    }
    for (int dt = 0; dt < 2; ++dt)
        for (int B : {1, 64, 512, 4096, 65536})
            for (int r : {1, 10, 100, 500})
                for (int c : {1, 10, 100, 500}) {
                    const size_t ws = qpx_batch_outer_workspace_elems(dt, B, r, c);
                    std::printf("# outer dt=%d B=%d r=%d c=%d ws=%zu\n", dt, B, r, c, ws);
                    qpx_batch_outer(dt, B, r, c, P(1), c > 1 ? P(2) : nullptr, P(3), P(4), 0.5, P(5), ws ? P(6) : nullptr, ws, nullptr);
                    qpx_dense_solve(dt, B, r, P(1), P(2), (int32_t*)P(3), nullptr);
                }
    return 0;
}
