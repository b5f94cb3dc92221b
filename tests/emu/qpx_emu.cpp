// tests/emu/qpx_emu.cpp -- libqpx_emu.so: the C ABI of include/qpx.h executed by host threads.
//
// TEST INFRASTRUCTURE ONLY (see tests/emu/qpx_platform.h).  Pointers are host pointers; the
// `stream` argument is ignored; workgroups run one after the other, each as QPX_EMU_THREADS
// (default 128 = two waves) fibers of the calling thread (pthreads with -DQPX_EMU_PTHREADS: the sanitizer
// drivers) over a heap-allocated "LDS".
#include <pthread.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/qpx.h"
#include "qpx_platform.h"  // the emulation header: defines QPX_PLATFORM_H, so the HIP one is skipped
#include "qpx_forms.h"
#include "qpx_kernels.h"
#include "qpx_grid.h"
#include "qpx_tile.h"
#include "qpx_prefac.h"
#include "qpx_reduce.h"
#include "qpx_big.h"
#include "qpx_big_polish.h"

// Extra bytes behind the emulated LDS block.  The sanitizer build uses 0 so that an index one element past
// the size the launcher computed is already a reported overflow.
#ifndef QPX_EMU_LDS_SLACK
#define QPX_EMU_LDS_SLACK 64
#endif

namespace qpx {

// QPX_EMU_LDS_BYTES shrinks the emulated LDS so that small problems exercise the
// "matrices stay in the HBM blob" code path.
inline size_t lds_budget_bytes()
{
    const char* e = std::getenv("QPX_EMU_LDS_BYTES");
    return e ? (size_t)std::atoll(e) : kMaxLdsBytes;
}

static int emu_threads()
{
    const char* e = std::getenv("QPX_EMU_THREADS");
    int nt = e ? std::atoi(e) : 128;
    if (nt < 64) nt = 64;
    return (nt / 64) * 64;
}

#ifdef QPX_EMU_PTHREADS
// The nt threads of a workgroup size live as long as the process: under ThreadSanitizer, creating and joining 256
// threads for every workgroup cost ~85 ms, most of a sanitizer run.  A launch is bracketed by the pool's two barriers
// (nt workers + the launching thread), which order it after everything before and before everything after, as
// pthread_create / pthread_join did; inside the launch only the kernel's own barriers order the threads.
struct WorkerPool;
struct WorkerArg {
    WorkerPool* pool;
    int t;
};

struct WorkerPool {
    int nt = 0;
    pthread_barrier_t start, done;
    void (*run)(const void* body, const Block& blk) = nullptr;
    const void* body = nullptr;
    EmuShared* sh = nullptr;
    bool quit = false;
    std::vector<WorkerArg> args;
    std::vector<pthread_t> th;
};

static void* worker_main(void* p)
{
    const WorkerArg* a = static_cast<const WorkerArg*>(p);
    WorkerPool* P = a->pool;
    for (;;) {
        pthread_barrier_wait(&P->start);
        if (P->quit) return nullptr;
        P->run(P->body, Block{a->t, P->nt, P->sh});
        pthread_barrier_wait(&P->done);
    }
}

static WorkerPool* pool_for(int nt)
{
    static struct Pools {
        std::vector<WorkerPool*> all;
        ~Pools()
        {
            for (WorkerPool* P : all) {
                P->quit = true;
                pthread_barrier_wait(&P->start);
                for (pthread_t t : P->th) pthread_join(t, nullptr);
                pthread_barrier_destroy(&P->start);
                pthread_barrier_destroy(&P->done);
                delete P;
            }
        }
    } pools;
    for (WorkerPool* P : pools.all)
        if (P->nt == nt) return P;
    auto* P = new WorkerPool;
    P->nt = nt;
    pthread_barrier_init(&P->start, nullptr, nt + 1);
    pthread_barrier_init(&P->done, nullptr, nt + 1);
    P->args.resize(nt);
    P->th.resize(nt);
    pthread_attr_t attr;
    pthread_attr_init(&attr);
    pthread_attr_setstacksize(&attr, 1 << 20);
    for (int t = 0; t < nt; ++t) {
        P->args[t] = WorkerArg{P, t};
        pthread_create(&P->th[t], &attr, worker_main, &P->args[t]);
    }
    pthread_attr_destroy(&attr);
    pools.all.push_back(P);
    return P;
}

// run `body(block)` for one workgroup
template <class Body> static void run_block(int nt, const Body& body)
{
    EmuShared sh;
    const int nw = nt / kWave;
    pthread_barrier_init(&sh.block_bar, nullptr, nt);
    std::vector<pthread_barrier_t> wb(nw);
    for (int w = 0; w < nw; ++w) pthread_barrier_init(&wb[w], nullptr, kWave);
    sh.wave_bar = wb.data();
    std::vector<unsigned long long> xchg(nt, 0);
    sh.xchg = xchg.data();
    std::vector<unsigned long long> xchg2(nt, 0);
    sh.xchg2 = xchg2.data();
    std::vector<double> xv((size_t)nt * 16, 0.0);
    sh.xv = xv.data();
    WorkerPool* P = pool_for(nt);
    P->run = [](const void* b, const Block& blk) { (*static_cast<const Body*>(b))(blk); };
    P->body = &body;
    P->sh = &sh;
    pthread_barrier_wait(&P->start);
    pthread_barrier_wait(&P->done);
    for (int w = 0; w < nw; ++w) pthread_barrier_destroy(&wb[w]);
    pthread_barrier_destroy(&sh.block_bar);
}
#else
// ---------------------------------------------------------------------------------------------- fibers
// The GPU threads of one workgroup as user-level contexts of the calling host thread.  A context is a stack pointer:
// qpx_fiber_switch pushes the callee-saved registers of the System V x86-64 ABI, stores the stack pointer, loads the
// other context's and pops its registers (nothing in the kernel bodies changes MXCSR or the x87 control word).
extern "C" void qpx_fiber_switch(void** save_sp, void* load_sp);
asm(R"(
    .text
    .globl qpx_fiber_switch
    .type qpx_fiber_switch,@function
qpx_fiber_switch:
    pushq %rbp
    pushq %rbx
    pushq %r12
    pushq %r13
    pushq %r14
    pushq %r15
    movq %rsp, (%rdi)
    movq %rsi, %rsp
    popq %r15
    popq %r14
    popq %r13
    popq %r12
    popq %rbx
    popq %rbp
    ret
    .size qpx_fiber_switch, .-qpx_fiber_switch
    .section .note.GNU-stack,"",@progbits
    .text
)");

struct Fiber {
    void* sp = nullptr;
    FiberBar* waits = nullptr;     // the barrier this fiber sleeps at (nullptr: runnable)
    unsigned gen = 0;              // ... and the generation it arrived in
    bool done = false;
};
struct FiberSched {
    int nt = 0, cur = 0, ndone = 0;
    void* main_sp = nullptr;
    Fiber* f = nullptr;
    void (*entry)(FiberSched*, int) = nullptr;   // runs the body of fiber `tid`
    const void* body = nullptr;
    EmuShared* sh = nullptr;
};
static thread_local FiberSched* g_sched = nullptr;

// next runnable fiber after `cur` in round-robin order; -1 = every live fiber sleeps at a barrier nobody can open
static int fiber_pick(FiberSched* s)
{
    for (int k = 1; k <= s->nt; ++k) {
        const int t = (s->cur + k) % s->nt;
        Fiber& f = s->f[t];
        if (f.done) continue;
        if (f.waits && f.waits->gen == f.gen) continue;
        return t;
    }
    return -1;
}
static void fiber_deadlock(FiberSched* s)
{
    std::fprintf(stderr, "qpx_emu: dead-lock -- %d of %d GPU threads have finished and the others wait at barriers that "
                         "not every thread reaches (divergent __syncthreads / wave barrier in a kernel body)\n", s->ndone, s->nt);
    std::abort();
}
void fiber_wait(FiberSched* s, FiberBar* b, int parties)
{
    if (++b->count == parties) {       // last arrival: open the next generation and keep running
        b->count = 0;
        ++b->gen;
        return;
    }
    Fiber& me = s->f[s->cur];
    me.waits = b;
    me.gen = b->gen;
    const int t = fiber_pick(s);
    if (t < 0) fiber_deadlock(s);
    const int from = s->cur;
    s->cur = t;
    qpx_fiber_switch(&s->f[from].sp, s->f[t].sp);
    s->f[from].waits = nullptr;        // resumed: the generation has moved on
}
extern "C" void qpx_fiber_entry()
{
    FiberSched* s = g_sched;
    const int tid = s->cur;
    s->entry(s, tid);
    s->f[tid].done = true;
    ++s->ndone;
    const int t = fiber_pick(s);
    void* dead;
    if (t < 0) {
        if (s->ndone != s->nt) fiber_deadlock(s);
        qpx_fiber_switch(&dead, s->main_sp);          // the workgroup has finished
    } else {
        s->cur = t;
        qpx_fiber_switch(&dead, s->f[t].sp);
    }
    std::abort();                                      // a finished fiber is never resumed
}

// run `body(block)` for one workgroup
template <class Body> static void run_block(int nt, const Body& body)
{
    constexpr size_t kStack = 1 << 20;
    EmuShared sh;
    const int nw = nt / kWave;
    std::vector<FiberBar> wb(nw);
    sh.wave_bar = wb.data();
    std::vector<unsigned long long> xchg(nt, 0);
    sh.xchg = xchg.data();
    std::vector<unsigned long long> xchg2(nt, 0);
    sh.xchg2 = xchg2.data();
    std::vector<double> xv((size_t)nt * 16, 0.0);
    sh.xv = xv.data();
    // stacks: untouched pages of a fresh allocation cost nothing, so 1 MiB each as for the pthreads
    static thread_local unsigned char* stacks = nullptr;      // kept for the life of the host thread
    static thread_local size_t stacks_bytes = 0;
    if (stacks_bytes < (size_t)nt * kStack + 64) {
        std::free(stacks);
        stacks_bytes = (size_t)nt * kStack + 64;
        stacks = static_cast<unsigned char*>(std::malloc(stacks_bytes));
        if (!stacks) std::abort();
    }
    std::vector<Fiber> fib(nt);
    FiberSched sc;
    sc.nt = nt;
    sc.f = fib.data();
    sc.body = &body;
    sc.sh = &sh;
    sc.entry = [](FiberSched* s, int tid) { (*static_cast<const Body*>(s->body))(Block{tid, s->nt, s->sh}); };
    sh.sched = &sc;
    const uintptr_t base = ((uintptr_t)stacks + 63) & ~(uintptr_t)63;
    for (int t = 0; t < nt; ++t) {
        // initial frame: six zeroed callee-saved registers, the entry point as the return address of the first
        // switch, and a null return address above it (the entry function never returns); the stack pointer at
        // the entry is then 8 mod 16, as after a call
        uintptr_t top = (base + (size_t)(t + 1) * kStack) & ~(uintptr_t)15;
        void** p = reinterpret_cast<void**>(top);
        *--p = nullptr;
        *--p = reinterpret_cast<void*>(&qpx_fiber_entry);
        for (int r = 0; r < 6; ++r) *--p = nullptr;
        fib[t].sp = p;
    }
    FiberSched* outer = g_sched;
    g_sched = &sc;
    sc.cur = 0;
    qpx_fiber_switch(&sc.main_sp, fib[0].sp);
    g_sched = outer;
    if (sc.ndone != nt) fiber_deadlock(&sc);
}
#endif

// every launch: a grid (B, gy) of workgroups, one after the other, each over a fresh zero-initialised "LDS"
template <class F> static int emu_grid(int B, int gy, int threads, size_t lds_bytes, const F& body)
{
    for (int y = 0; y < gy; ++y)
        for (int qp = 0; qp < B; ++qp) {
            std::vector<unsigned char> lds(lds_bytes + QPX_EMU_LDS_SLACK);
            unsigned char* base = lds.data();
            run_block(threads, [&](const Block& b) { body(b, qp, y, base); });
        }
    return QPX_OK;
}
// one workgroup per QP, the LDS as the kernel's type
template <class T, class F> static int emu_per_qp(int B, int threads, size_t lds_bytes, const F& body)
{
    return emu_grid(B, 1, threads, lds_bytes, [&](const Block& b, int qp, int, unsigned char* l) { body(b, qp, reinterpret_cast<T*>(l)); });
}

template <class T, int NBL> int launch_sweep(const PrefactorArgs<T>& a, size_t lds_bytes, void*)
{
    return emu_per_qp<T>(a.B, 256, lds_bytes, [&](const Block& b, int qp, T* lds) { sweep_body<T, NBL>(b, a, qp, lds); });
}
template <int NBN, bool kEq> int launch_prefac_tile(const PrefactorArgs<double>& a, size_t lds_bytes, void*)
{
    return emu_per_qp<double>(a.B, 256, lds_bytes, [&](const Block& b, int qp, double* lds) { prefac_tile_body<NBN, kEq>(b, a, qp, lds); });
}
template <class T, int NBL, int NS> int launch_ipm_grid(const IpmArgs<T>& a, size_t lds_bytes, void*)
{
    return emu_per_qp<T>(a.B, 256, lds_bytes, [&](const Block& b, int qp, T* lds) { ipm_grid_body<T, 16, NBL, NS>(b, a, qp, lds); });
}
template <class T, int NBL, int NS> int launch_ipm_grid8(const IpmArgs<T>& a, size_t lds_bytes, void*)
{
    return emu_per_qp<T>(a.B, 64, lds_bytes, [&](const Block& b, int qp, T* lds) { ipm_grid_body<T, 8, NBL, NS>(b, a, qp, lds); });
}
template <int NBL, int NW, int NS, bool CH> int launch_ipm_tile(const IpmArgs<double>& a, size_t lds_bytes, void*)
{
    return emu_per_qp<double>(a.B, 64 * NW, lds_bytes, [&](const Block& b, int qp, double* lds) { ipm_tile_body<NBL, NW, NS, CH>(b, a, qp, lds); });
}
template <int NBL, int NW, bool kBw, bool CH> int launch_kkt_tile(const KktArgs<double>& a, size_t lds_bytes, void*)
{
    return emu_per_qp<double>(a.B, 64 * NW, lds_bytes, [&](const Block& b, int qp, double* lds) { kkt_tile_body<NBL, NW, kBw, CH>(b, a, qp, lds); });
}
template <class T, int NBL, bool kBw> int launch_kkt_grid(const KktArgs<T>& a, size_t lds_bytes, void*)
{
    return emu_per_qp<T>(a.B, 256, lds_bytes, [&](const Block& b, int qp, T* lds) { kkt_grid_body<T, 16, NBL, kBw>(b, a, qp, lds); });
}
template <class T, int NBL> int launch_polish_grid(const PolishArgs<T>& a, size_t lds_bytes, void*)
{
    return emu_per_qp<T>(a.B, 256, lds_bytes, [&](const Block& b, int qp, T* lds) { polish_grid_body<T, 16, NBL>(b, a, qp, lds); });
}
template <int NBL, int NW, bool CH> int launch_polish_tile(const PolishArgs<double>& a, size_t lds_bytes, void*)
{
    return emu_per_qp<double>(a.B, 64 * NW, lds_bytes, [&](const Block& b, int qp, double* lds) { polish_mat_body<double, TileMat<NBL, NW, CH>>(b, a, qp, lds); });
}

// the large-QP family
template <class T> int launch_big_pack(const BigPackArgs<T>& a, int gy, void*)
{
    return emu_grid(a.B, gy, 256, 0, [&](const Block& b, int qp, int y, unsigned char*) { big_pack_body<T>(b, a, qp, y); });
}
template <class T> int launch_big_panel(const BigPanelArgs<T>& a, void*)
{
    return emu_per_qp<T>(a.B, 256, big_panel_lds_elems() * sizeof(T), [&](const Block& b, int qp, T* lds) { big_panel_body<T>(b, a, qp, lds); });
}
template <class T> int launch_big_gemm(const BigGemmArgs<T>& a, void*)
{
    return emu_grid(a.B, a.nti * a.ntj, 256, big_gemm2_lds_elems<T>(a.fuse != 0, a.mirror != 0) * sizeof(T), [&](const Block& b, int qp, int y, unsigned char* l) { big_gemm2_body<T, true>(b, a, qp, y, reinterpret_cast<T*>(l)); });
}
template <class T> int launch_big_trsv(const BigTrsvArgs<T>& a, void*)
{
    return emu_per_qp<T>(a.B, 64 * kTrsvNW, big_trsv_lds_elems(a.nb * kBB) * sizeof(T), [&](const Block& b, int qp, T* lds) {
        if (a.nb > 8) big_trsv_body<T, true>(b, a, qp, lds);
        else big_trsv_body<T, false>(b, a, qp, lds);
    });
}
template <class T> int launch_big_gemv(const BigGemvArgs<T>& a, void*)
{
    const int outs = a.trans ? a.cols : a.rows;
    return emu_grid(a.B, (outs + kBB - 1) / kBB, 256, big_gemv_lds_elems(a.trans ? a.rows : a.cols) * sizeof(T), [&](const Block& b, int qp, int y, unsigned char* l) { big_gemv_body<T>(b, a, qp, y, reinterpret_cast<T*>(l)); });
}
template <class T> int launch_big_symv(const BigSymvArgs<T>& a, void*)
{
    return emu_grid(a.B, a.stage == 0 ? a.ld / kBB : 1, 256, big_symv_lds_elems() * sizeof(T), [&](const Block& b, int qp, int y, unsigned char* l) { big_symv_body<T>(b, a, qp, y, reinterpret_cast<T*>(l)); });
}
template <class T> int launch_big_vec(const BigVecArgs<T>& a, void*)
{
    return emu_grid(a.B, 1, 256, 0, [&](const Block& b, int qp, int, unsigned char*) { big_vec_body<T>(b, a, qp); });
}
template <class T> int launch_big_kkt(const BigKktArgs<T>& a, int gy, void*)
{
    return emu_grid(a.B, gy, 256, 0, [&](const Block& b, int qp, int y, unsigned char*) { big_kkt_body<T>(b, a, qp, y); });
}
template <class T> int launch_big_phase(const BigPhaseArgs<T>& a, void*)
{
    return big_ns_form(big_pad(a.m) / kWave, [&](auto ns) {
        return emu_grid(a.B, 1, 64, 0, [&](const Block& b, int qp, int, unsigned char*) { big_phase_body<T, decltype(ns)::value>(b, a, qp); });
    });
}
template <class T> int launch_big_solve(const BigSolveArgs<T>& a, void*)
{
    return big_ns_form(big_pad(a.ph.m) / kWave, [&](auto ns) {
        return emu_per_qp<T>(a.t.B, 64 * kTrsvNW, big_trsv_lds_elems(a.t.nb * kBB) * sizeof(T), [&](const Block& b, int qp, T* lds) { big_solve_body<T, decltype(ns)::value>(b, a, qp, lds); });
    });
}
template <class T> int launch_big_polish(const BigPolishArgs<T>& a, void*)
{
    const BigLayout L = big_layout(a.n, a.m, a.q);
    return emu_per_qp<double>(a.B, 64 * kBigPolWaves, big_polish_lds_doubles(L.VP) * sizeof(double), [&](const Block& b, int qp, double* lds) { big_polish_body<T>(b, a, qp, lds); });
}
template <class T> int launch_big_diag(const BigDiagArgs<T>& a, void*)
{
    return big_ns_form(big_pad(a.ph.m) / kWave, [&](auto ns) {
        return emu_per_qp<T>(a.p.B, 256, big_panel_lds_elems() * sizeof(T), [&](const Block& b, int qp, T* lds) { big_diag_body<T, decltype(ns)::value>(b, a, qp, lds); });
    });
}

template <class T> int launch_batch_outer(const OuterArgs<T>& a, int tiles, void*)
{
    for (int ch = 0; ch < a.chunks; ++ch)
        for (int t = 0; t < tiles; ++t) {
            std::vector<T> lds((size_t)kOuterWaves * 256);
            run_block(64 * kOuterWaves, [&](const Block& b) { batch_outer_body<T>(b, a, t, ch, lds.data()); });
        }
    if (a.chunks > 1)
        for (int t = 0; t < tiles; ++t) run_block(256, [&](const Block& b) { batch_outer_sum_body<T>(b, a, t); });
    return QPX_OK;
}

template <class T> int launch_dense_solve(const DenseSolveArgs<T>& a, void*)
{
    for (int qp = 0; qp < a.B; ++qp) {
        std::vector<T> lds(dense_solve_lds_elems(a.k));
        run_block(256, [&](const Block& b) { dense_solve_body<T>(b, a, qp, lds.data()); });
    }
    return QPX_OK;
}

// side streams: launches are synchronous here, so the parts of a batch simply run one after the other
int stream_fork(void* caller, int nside, void** side, int, int = 0)
{
    for (int i = 0; i < nside; ++i) side[i] = caller;
    return QPX_OK;
}
int stream_join(void*, int, void* const*, int = 0) { return QPX_OK; }

}  // namespace qpx

#include "qpx_api.inc"

// test hook: force the "matrices in HBM" code path regardless of size
extern "C" int qpx_emu_marker(void) { return 1; }
