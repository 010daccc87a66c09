/*
 * selfcheck.cc -- kernels of our own that check the stand-in runtime itself (tests/test_reference_host_cpu.py).
 * No reference text.  They are written the way the reference's kernels are, against the same stand-in headers.
 */
#include <torch/extension.h>

#include <cuda.h>
#include <cuda_runtime.h>

namespace {

/* Every thread writes its own slot of the dynamic shared memory, then reads its right-hand neighbour's (cyclic).
 * Threads past `n` return before the barrier, as the guards of real kernels do.  Without a working barrier a thread
 * reads a slot that has not been written yet (forward order: all but the last) and sees the poison. */
template <typename scalar_t, bool with_barrier>
__global__ void neighbour_kernel(torch::PackedTensorAccessor<scalar_t, 2, torch::RestrictPtrTraits, size_t> out, uint32_t n) {
    const uint32_t t = threadIdx.x + threadIdx.y * blockDim.x;
    const uint32_t live = n < blockDim.x * blockDim.y ? n : blockDim.x * blockDim.y;
    if (t >= n) {
        return;
    }
    scalar_t *slots = static_cast<scalar_t *>(refhost::block_shared());
    slots[t] = static_cast<scalar_t>(1000 * (blockIdx.x + 1) + t);
    if (with_barrier) {
        __syncthreads();
    }
    out[blockIdx.x][t] = slots[(t + 1) % live];
}

}  // namespace

/* out: [blocks][threads_x * threads_y] floats, cells of threads >= n keep the poison.  Returns 0. */
extern "C" int ref_host_selfcheck_barrier(int blocks, int threads_x, int threads_y, int n, int with_barrier, float poison,
                                          int reverse, float *out) {
    refhost::set_poison(poison);
    refhost::set_reverse(reverse != 0);
    const int per_block = threads_x * threads_y;
    torch::Tensor t = torch::empty({blocks, per_block});
    const dim3 grid(blocks), block(threads_x, threads_y);
    auto acc = t.packed_accessor<float, 2, torch::RestrictPtrTraits, size_t>();
    if (with_barrier) {
        refhost::launch(refhost::launch_cfg(grid, block, per_block * sizeof(float)), neighbour_kernel<float, true>, acc, n);
    } else {
        refhost::launch(refhost::launch_cfg(grid, block, per_block * sizeof(float)), neighbour_kernel<float, false>, acc, n);
    }
    for (int i = 0; i < blocks * per_block; i++) out[i] = t.data_ptr<float>()[i];
    return 0;
}

/* A [rows][cols] tensor filled with 1..rows*cols; reads element [row][col] through the accessor with SIGNED int32
 * indices, as the reference's kernels index (a negative row reaches whole rows before the base: the guard band). */
extern "C" float ref_host_selfcheck_read(int rows, int cols, int32_t row, int32_t col, float poison) {
    refhost::set_poison(poison);
    torch::Tensor t = torch::empty({rows, cols});
    for (int i = 0; i < rows * cols; i++) t.data_ptr<float>()[i] = static_cast<float>(i + 1);
    auto acc = t.packed_accessor<float, 2, torch::RestrictPtrTraits, size_t>();
    return acc[row][col];
}

/* The types the semantics hang on: 1 when a signed -1 compares as "not below" an accessor's size() (size_t), the
 * built-in indices are unsigned and Tensor::size() is a signed 64-bit integer. */
extern "C" int ref_host_selfcheck_types(void) {
    torch::Tensor t = torch::empty({2, 3});
    auto acc = t.packed_accessor<float, 2, torch::RestrictPtrTraits, size_t>();
    const int32_t minus_one = -1;
    const bool wraps = minus_one >= acc.size(0);
    const bool unsigned_idx = std::is_same<decltype(threadIdx.x), unsigned>::value && std::is_same<decltype(blockDim.y), unsigned>::value &&
                              std::is_same<decltype(blockIdx.z * blockDim.z + threadIdx.z), unsigned>::value;
    const bool sizes = std::is_same<decltype(acc.size(0)), size_t>::value && std::is_same<decltype(t.size(0)), int64_t>::value;
    return (wraps ? 1 : 0) | (unsigned_idx ? 2 : 0) | (sizes ? 4 : 0);
}
