/*
 * runner.cc -- the grid runner behind ref_host.h (our own code; test infrastructure only).
 *
 * One block at a time.  Every thread of the block is a ucontext fiber on the calling OS thread.  A round resumes
 * every live fiber once, in thread order (x fastest, as the hardware numbers them) or last to first; a fiber runs
 * until it returns or reaches __syncthreads(), so at the end of a round every live thread has arrived at the barrier
 * or has returned, and the next round releases them together.  A thread that returns before a barrier simply stops
 * taking part, which is what the hardware does with the reference's early-return guards.
 * The built-in index variables are plain globals, rewritten before every resume.
 */
#include "ref_host.h"

#include <ucontext.h>

#include <cstring>

uint3 threadIdx, blockIdx;
dim3 blockDim, gridDim;

namespace refhost {

namespace {

float g_poison = 0.0f;
bool g_reverse = false;

const size_t kStackBytes = 64 * 1024;

struct fiber {
    ucontext_t ctx;
    uint3 tid;
    bool done;
};

ucontext_t g_scheduler;
fiber *g_current = nullptr;
const std::function<void()> *g_body = nullptr;
std::vector<float> g_shared;

void fiber_main() {
    (*g_body)();
    g_current->done = true;
    swapcontext(&g_current->ctx, &g_scheduler);
}

}  // namespace

void set_poison(float v) { g_poison = v; }
float poison() { return g_poison; }
void set_reverse(bool r) { g_reverse = r; }
bool reverse() { return g_reverse; }

void *block_shared() { return g_shared.data(); }

void fail(const char *what, const char *detail) {
    std::fprintf(stderr, "ref_host: %s: %s\n", what, detail);
    std::abort();
}

void run_grid(const launch_cfg &cfg, const std::function<void()> &thread_body) {
    if (g_current) fail("run_grid", "nested launch");
    const size_t nthreads = static_cast<size_t>(cfg.block.x) * cfg.block.y * cfg.block.z;
    const size_t nblocks = static_cast<size_t>(cfg.grid.x) * cfg.grid.y * cfg.grid.z;
    if (nthreads == 0 || nthreads > 1024) fail("run_grid", "block of 0 or more than 1024 threads");
    std::vector<fiber> fibers(nthreads);
    std::vector<char> stacks(nthreads * kStackBytes);
    g_body = &thread_body;
    gridDim = cfg.grid;
    blockDim = cfg.block;
    g_shared.resize((cfg.shared_bytes + sizeof(float) - 1) / sizeof(float) + 1);

    for (size_t bi = 0; bi < nblocks; bi++) {
        const size_t b = g_reverse ? nblocks - 1 - bi : bi;
        blockIdx.x = static_cast<unsigned>(b % cfg.grid.x);
        blockIdx.y = static_cast<unsigned>((b / cfg.grid.x) % cfg.grid.y);
        blockIdx.z = static_cast<unsigned>(b / (static_cast<size_t>(cfg.grid.x) * cfg.grid.y));
        for (float &v : g_shared) v = g_poison;
        for (size_t t = 0; t < nthreads; t++) {
            fiber &f = fibers[t];
            f.tid.x = static_cast<unsigned>(t % cfg.block.x);
            f.tid.y = static_cast<unsigned>((t / cfg.block.x) % cfg.block.y);
            f.tid.z = static_cast<unsigned>(t / (static_cast<size_t>(cfg.block.x) * cfg.block.y));
            f.done = false;
            getcontext(&f.ctx);
            f.ctx.uc_stack.ss_sp = stacks.data() + t * kStackBytes;
            f.ctx.uc_stack.ss_size = kStackBytes;
            f.ctx.uc_link = &g_scheduler;
            makecontext(&f.ctx, fiber_main, 0);
        }
        size_t live = nthreads;
        while (live) {
            for (size_t ti = 0; ti < nthreads; ti++) {
                fiber &f = fibers[g_reverse ? nthreads - 1 - ti : ti];
                if (f.done) continue;
                g_current = &f;
                threadIdx = f.tid;
                swapcontext(&g_scheduler, &f.ctx);
                if (f.done) live--;
            }
        }
        g_current = nullptr;
    }
    g_body = nullptr;
}

}  // namespace refhost

void __syncthreads() {
    using namespace refhost;
    if (!g_current) fail("__syncthreads", "called outside a kernel");
    fiber *self = g_current;
    swapcontext(&self->ctx, &g_scheduler);
    /* resumed: the scheduler has restored threadIdx for this fiber */
}
