/*
 * ref_host.h -- host stand-in for the sliver of CUDA and libtorch that the reference's stereo path uses.
 *
 * TEST INFRASTRUCTURE ONLY, and our own code: no text of the reference is in this directory.  oracle/build_ref.py
 * compiles the reference's own sources against these headers with g++, so the program that runs is the reference's
 * text and not a reading of it.  What is mirrored is what the semantics hang on:
 *   - threadIdx/blockIdx/blockDim/gridDim and dim3 have `unsigned` members;
 *   - the accessor's size() returns its index type (size_t here), its operator[] takes that type and multiplies by a
 *     stride of that type, so a negative int32_t index wraps into a negative element offset as on the device;
 *   - Tensor::size() returns int64_t;
 *   - torch::empty() initialises nothing the caller could rely on: body, guard bands and the dynamic shared memory of
 *     every block are filled with one run-time "poison" float, so a read of uninitialised or out-of-bounds memory
 *     shows as a dependence on that value;
 *   - every tensor sits between two guard bands of at least twice its own element count; a dereference outside
 *     body + guards aborts with a message instead of touching foreign memory.
 * The grid runner (runner.cc) executes one block at a time with the block's threads as ucontext fibers;
 * __syncthreads() yields until every live thread of the block has arrived or returned.
 */
#ifndef REF_HOST_H
#define REF_HOST_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <initializer_list>
#include <memory>
#include <type_traits>
#include <vector>

/* ---- CUDA side ------------------------------------------------------------------------------------------------ */
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __align__(n)

struct uint3 {
    unsigned x, y, z;
};

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};

extern uint3 threadIdx, blockIdx;
extern dim3 blockDim, gridDim;

void __syncthreads();

namespace refhost {

/* Run-time switches of one run (set by the driver before the first torch::empty). */
void set_poison(float v);
float poison();
void set_reverse(bool last_to_first);
bool reverse();

struct launch_cfg {
    dim3 grid, block;
    size_t shared_bytes;
    launch_cfg(dim3 g, dim3 b, size_t s = 0) : grid(g), block(b), shared_bytes(s) {}
};

/* The current block's dynamic shared memory (poison-filled at the start of every block). */
void *block_shared();

/* Runs `thread_body` once per thread of the grid, block by block; see runner.cc. */
void run_grid(const launch_cfg &cfg, const std::function<void()> &thread_body);

/* kernel<<<grid, block[, shared]>>>(args...) becomes launch(launch_cfg(grid, block[, shared]), kernel, args...):
 * the arguments are evaluated once and converted to the kernel's parameter types, as a launch does. */
template <typename... P, typename... A>
void launch(const launch_cfg &cfg, void (*kernel)(P...), A &&...args) {
    std::function<void(P...)> k = kernel;
    std::function<void()> body = std::bind(k, static_cast<P>(args)...);
    run_grid(cfg, body);
}

[[noreturn]] void fail(const char *what, const char *detail);

}  // namespace refhost

/* ---- libtorch side -------------------------------------------------------------------------------------------- */
#define TORCH_CHECK(cond, ...)                                   \
    do {                                                         \
        if (!(cond)) refhost::fail("TORCH_CHECK failed", #cond); \
    } while (0)

#define AT_DISPATCH_FLOATING_TYPES(TYPE, NAME, ...)                              \
    do {                                                                         \
        if (!(TYPE).is_float32()) refhost::fail(NAME, "only float32 is built");  \
        using scalar_t = float;                                                  \
        (__VA_ARGS__)();                                                         \
    } while (0)

namespace torch {

template <typename T>
struct RestrictPtrTraits {
    typedef T *__restrict__ PtrType;
};

enum ScalarType { kFloat32 };
enum DeviceType { kCUDA };

struct Device {
    DeviceType kind;
    bool is_cuda() const { return kind == kCUDA; }
};

struct DeprecatedTypeProperties {
    ScalarType scalar;
    bool is_float32() const { return scalar == kFloat32; }
};

struct TensorOptions {
    ScalarType scalar = kFloat32;
    DeviceType dev = kCUDA;
    TensorOptions dtype(ScalarType s) const {
        TensorOptions o = *this;
        o.scalar = s;
        return o;
    }
    TensorOptions device(DeviceType d) const {
        TensorOptions o = *this;
        o.dev = d;
        return o;
    }
};

struct IntArrayRef {
    std::vector<int64_t> v;
    IntArrayRef(std::initializer_list<int64_t> l) : v(l) {}
};

/* An accessor level: the data pointer moves by stride * index in the index type's modular arithmetic. */
template <typename T, size_t N, template <typename U> class PtrTraits, typename index_t>
class TensorAccessor {
public:
    TensorAccessor(T *data, const index_t *sizes, const index_t *strides, const T *lo, const T *hi)
        : data_(data), sizes_(sizes), strides_(strides), lo_(lo), hi_(hi) {}
    index_t size(index_t i) const { return sizes_[i]; }
    index_t stride(index_t i) const { return strides_[i]; }
    TensorAccessor<T, N - 1, PtrTraits, index_t> operator[](index_t i) const {
        return TensorAccessor<T, N - 1, PtrTraits, index_t>(step(data_, strides_[0], i), sizes_ + 1, strides_ + 1, lo_, hi_);
    }
    static T *step(T *p, index_t stride, index_t i) {
        return reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(p) + static_cast<uintptr_t>(stride * i) * sizeof(T));
    }

protected:
    T *data_;
    const index_t *sizes_, *strides_;
    const T *lo_, *hi_;
};

template <typename T, template <typename U> class PtrTraits, typename index_t>
class TensorAccessor<T, 1, PtrTraits, index_t> {
public:
    TensorAccessor(T *data, const index_t *sizes, const index_t *strides, const T *lo, const T *hi)
        : data_(data), sizes_(sizes), strides_(strides), lo_(lo), hi_(hi) {}
    index_t size(index_t i) const { return sizes_[i]; }
    index_t stride(index_t i) const { return strides_[i]; }
    T &operator[](index_t i) const {
        T *p = TensorAccessor<T, 2, PtrTraits, index_t>::step(data_, strides_[0], i);
        if (p < lo_ || p >= hi_) refhost::fail("accessor", "element outside the tensor and its guard bands");
        return *p;
    }

protected:
    T *data_;
    const index_t *sizes_, *strides_;
    const T *lo_, *hi_;
};

template <typename T, size_t N, template <typename U> class PtrTraits, typename index_t>
class PackedTensorAccessor {
public:
    PackedTensorAccessor(T *data, const int64_t *sizes, const int64_t *strides, const T *lo, const T *hi)
        : data_(data), lo_(lo), hi_(hi) {
        for (size_t i = 0; i < N; i++) {
            sizes_[i] = static_cast<index_t>(sizes[i]);
            strides_[i] = static_cast<index_t>(strides[i]);
        }
    }
    index_t size(index_t i) const { return sizes_[i]; }
    index_t stride(index_t i) const { return strides_[i]; }
    template <size_t M = N>
    typename std::enable_if<(M > 1), TensorAccessor<T, N - 1, PtrTraits, index_t>>::type operator[](index_t i) const {
        return TensorAccessor<T, N - 1, PtrTraits, index_t>(TensorAccessor<T, N, PtrTraits, index_t>::step(data_, strides_[0], i),
                                                            sizes_ + 1, strides_ + 1, lo_, hi_);
    }
    template <size_t M = N>
    typename std::enable_if<(M == 1), T &>::type operator[](index_t i) const {
        T *p = TensorAccessor<T, 2, PtrTraits, index_t>::step(data_, strides_[0], i);
        if (p < lo_ || p >= hi_) refhost::fail("accessor", "element outside the tensor and its guard bands");
        return *p;
    }

private:
    T *data_;
    index_t sizes_[N], strides_[N];
    const T *lo_, *hi_;
};

class Tensor {
public:
    Tensor() {}
    Tensor(const IntArrayRef &shape, const TensorOptions &options) : sizes_(shape.v), options_(options) {
        size_t n = 1;
        for (int64_t s : sizes_) n *= static_cast<size_t>(s);
        strides_.assign(sizes_.size(), 1);
        for (size_t i = sizes_.size(); i-- > 1;) strides_[i - 1] = strides_[i] * sizes_[i];
        numel_ = n;
        guard_ = 2 * n < 4096 ? 4096 : 2 * n;
        store_ = std::make_shared<std::vector<float>>(numel_ + 2 * guard_, refhost::poison());
    }
    int64_t size(int64_t d) const { return sizes_.at(static_cast<size_t>(d < 0 ? d + dim() : d)); }
    int64_t dim() const { return static_cast<int64_t>(sizes_.size()); }
    int64_t numel() const { return static_cast<int64_t>(numel_); }
    bool is_contiguous() const { return true; }
    Device device() const { return Device{options_.dev}; }
    DeprecatedTypeProperties type() const { return DeprecatedTypeProperties{options_.scalar}; }
    template <typename T>
    T *data_ptr() const {
        static_assert(std::is_same<T, float>::value, "float32 only");
        return store_->data() + guard_;
    }
    template <typename T, size_t N, template <typename U> class PtrTraits, typename index_t>
    PackedTensorAccessor<T, N, PtrTraits, index_t> packed_accessor() const {
        if (sizes_.size() != N) refhost::fail("packed_accessor", "rank mismatch");
        float *lo = store_->data();
        return PackedTensorAccessor<T, N, PtrTraits, index_t>(data_ptr<T>(), sizes_.data(), strides_.data(), lo, lo + store_->size());
    }

private:
    std::vector<int64_t> sizes_, strides_;
    TensorOptions options_;
    size_t numel_ = 0, guard_ = 0;
    std::shared_ptr<std::vector<float>> store_;
};

inline Tensor empty(IntArrayRef shape, const TensorOptions &options = TensorOptions()) { return Tensor(shape, options); }

}  // namespace torch

#endif
