// Per-system storage for kernels that run one system per thread: the include path and names of the reference's
// src/misc/BoundaryValueProblem/BVPMemory.cuh, written for this build.  The reference's doubly periodic solvers lay their per-wave-number
// scratch (potential, first and second derivative coefficients) out with these classes: register every array once on the host, allocate
// getRequestedStorageBytes() bytes, and inside the kernel ask a StorageRetriever for system `instance`'s view of each array.
// Element i of system s of an array sits at s + numberCopies i, so the threads of a wave touch consecutive addresses.
#pragma once
#include <cstddef>
#include <hip/hip_runtime.h>
#include <iterator>

namespace uammd {
namespace BVP {

template <class T> struct StorageHandle {
  using value_type = T;
  using pointer = T *;
  size_t offset;        // bytes from the start of the block
  int numberElements;   // per system
};

class StorageRegistration {
  size_t allocationSize = 0;
  int numberCopies;

public:
  StorageRegistration(int numberCopies) : numberCopies(numberCopies) {}

  // numberElements values of type T for each of the systems, aligned to sizeof(T)
  template <class T> StorageHandle<T> registerStorageRequirement(int numberElements) {
    const size_t misaligned = allocationSize % sizeof(T);
    if (misaligned) allocationSize += sizeof(T) - misaligned;
    StorageHandle<T> handle{allocationSize, numberElements};
    allocationSize += sizeof(T) * (size_t)numberCopies * (size_t)numberElements;
    return handle;
  }

  size_t getRequestedStorageBytes() const { return allocationSize; }
};

// Random access over one system's elements of an interleaved array.
template <class T> class Iterator {
  T *base;
  int stride;

public:
  using value_type = T;
  using reference = T &;
  using pointer = T *;
  using difference_type = std::ptrdiff_t;
  using iterator_category = std::random_access_iterator_tag;
  __host__ __device__ Iterator(T *base, int stride) : base(base), stride(stride) {}
  __host__ __device__ T &operator[](difference_type i) const { return base[i * stride]; }
  __host__ __device__ T &operator*() const { return *base; }
  __host__ __device__ Iterator operator+(difference_type i) const { return Iterator(base + i * stride, stride); }
  __host__ __device__ Iterator operator-(difference_type i) const { return Iterator(base - i * stride, stride); }
  __host__ __device__ Iterator &operator+=(difference_type i) { base += i * stride; return *this; }
  __host__ __device__ Iterator &operator++() { base += stride; return *this; }
  __host__ __device__ difference_type operator-(const Iterator &o) const { return (base - o.base) / stride; }
  __host__ __device__ bool operator==(const Iterator &o) const { return base == o.base; }
  __host__ __device__ bool operator!=(const Iterator &o) const { return base != o.base; }
};

class StorageRetriever {
  char *raw = nullptr;
  int numberCopies;
  int instance;

public:
  __host__ __device__ StorageRetriever(int numberCopies, int instance, char *ptr) : raw(ptr), numberCopies(numberCopies), instance(instance) {}

  template <class T> __host__ __device__ Iterator<T> retrieveStorage(const StorageHandle<T> &handle) const {
    return Iterator<T>(reinterpret_cast<T *>(raw + handle.offset) + instance, numberCopies);
  }
};

}  // namespace BVP
}  // namespace uammd
