// Topology-only tables of the torch-operator shim, written once for every operator family that needs one:
//   * PinnedLruCache -- a table is built once per index tensor and looked up by the tensor's IDENTITY and VERSION, never
//     by its contents (hashing them would synchronise).  An in-place edit bumps the version counter and misses.  Each
//     entry pins its tensor, so that a recycled allocation cannot alias a stale entry.  128 entries, least recently used
//     out first.  Every family keeps its own instance: entries and counters are not shared.
//   * build_chunked_csr -- the CSR of an index tensor's incidence (who names row r?) and the chunk list of its rows, built
//     with ATen where the tensor lives.
#pragma once
#include "common.hpp"

#include <hip/hip_runtime_api.h>

#include <list>
#include <mutex>
#include <string>
#include <unordered_map>

namespace drtk_amd_torch {

using CacheKey = std::vector<int64_t>;
struct CacheKeyHash {
  size_t operator()(const CacheKey& k) const {
    uint64_t h = 1469598103934665603ull; // FNV-1a over the fields
    for (int64_t x : k) {
      h ^= static_cast<uint64_t>(x);
      h *= 1099511628211ull;
    }
    return static_cast<size_t>(h);
  }
};

// Which tensor, seen how, in which state.  A family appends what else its table depends on (a vertex count, ...).
inline void append_tensor_identity(CacheKey& k, const Tensor& t) {
  const auto address = [](const void* p) { return static_cast<int64_t>(reinterpret_cast<uintptr_t>(p)); };
  k.reserve(k.size() + 2 * t.dim() + 12); // one allocation on the hit path: these fields and a few of the family's
  k.insert(k.end(), {static_cast<int64_t>(t.device().type()), static_cast<int64_t>(t.device().index()),
                     address(t.storage().unsafeGetStorageImpl()), address(t.data_ptr()), t.dim()});
  k.insert(k.end(), t.sizes().begin(), t.sizes().end());
  k.insert(k.end(), t.strides().begin(), t.strides().end());
  k.insert(k.end(), {t.storage_offset(), static_cast<int64_t>(t.scalar_type()),
                     static_cast<int64_t>(t.unsafeGetTensorImpl()->version_counter().current_version())});
}

// A build reads numbers back and allocates: not capturable.  `table`: "vertex incidence of this index tensor";
// `arg`: the operator's argument the table is built from.
inline void check_not_capturing(const at::Device& device, const char* op, const char* table, const char* arg) {
  if (!device.is_cuda()) return;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  const hipStream_t s = c10::hip::getCurrentHIPStream(device.index()).stream();
  TORCH_CHECK(hipStreamIsCapturing(s, &st) != hipSuccess || st == hipStreamCaptureStatusNone, op, "(): the ", table,
              " is not cached yet, and it cannot be built while the stream is being captured -- run the op once with the "
              "same ", arg, " before the capture");
}

template <class Value>
class PinnedLruCache {
 public:
  static constexpr size_t kCapacity = 128;
  // `build` runs outside the lock, and only on a miss: whatever must hold before a build (check_not_capturing, argument
  // checks) goes into it.  A build that throws caches nothing and counts nothing.  `pin` may be undefined.
  template <class BuildFn>
  Value get(const CacheKey& key, const Tensor& pin, BuildFn&& build) {
    {
      std::lock_guard<std::mutex> lock(mu_);
      if (const Value* hit = touch(key)) {
        ++hits_;
        return *hit;
      }
    }
    Value built = build();
    std::lock_guard<std::mutex> lock(mu_);
    if (const Value* hit = touch(key)) return *hit; // a racing identical miss got there first
    ++misses_;
    while (lru_.size() >= kCapacity) {
      index_.erase(lru_.back().key);
      lru_.pop_back();
    }
    lru_.push_front(Entry{key, pin, built});
    index_.emplace(key, lru_.begin());
    return built;
  }
  std::vector<int64_t> stats() {
    std::lock_guard<std::mutex> lock(mu_);
    return {hits_, misses_, static_cast<int64_t>(lru_.size())};
  }
  void clear() {
    std::lock_guard<std::mutex> lock(mu_);
    lru_.clear();
    index_.clear();
    hits_ = misses_ = 0;
  }

 private:
  struct Entry {
    CacheKey key;
    Tensor pinned;
    Value value;
  };
  const Value* touch(const CacheKey& key) {
    const auto it = index_.find(key);
    if (it == index_.end()) return nullptr;
    lru_.splice(lru_.begin(), lru_, it->second);
    return &it->second->value;
  }
  std::mutex mu_;
  std::list<Entry> lru_;
  std::unordered_map<CacheKey, typename std::list<Entry>::iterator, CacheKeyHash> index_;
  int64_t hits_ = 0, misses_ = 0;
};

// ---------------------------------------------------------------------------------------------
// CSR over `rows` rows of the int64 `keys` [E] (a key == rows belongs to no row and sorts behind every row), and the list
// of its chunks: `chunk` entries each, of every row or only of the rows longer than `chunk`.  Stable sort of the keys (the
// permutation is then ascending within a row), searchsorted for the row starts.  One host read per build: the chunk
// count (a launch size) and the range of `range_of`, which the caller holds against what its kernels may index.
// ---------------------------------------------------------------------------------------------
struct ChunkedCsr {
  Tensor crow, chunk_ptr, chunk_begin, chunk_row; // int32 [rows+1], [rows+1], [C], [C]
  Tensor perm; // int64 [E], the stable sort's permutation
  int64_t C = 0, lo = 0, hi = 0; // chunks; min / max of `range_of` (0 when E == 0)

  // what the kernels read of it travels through autograd contexts as saved data
  void save(AutogradContext* ctx, const std::string& k) const {
    ctx->saved_data[k + "crow"] = crow;
    ctx->saved_data[k + "chunk_ptr"] = chunk_ptr;
    ctx->saved_data[k + "chunk_begin"] = chunk_begin;
    ctx->saved_data[k + "chunk_row"] = chunk_row;
    ctx->saved_data[k + "chunks"] = C;
  }
  static ChunkedCsr load(AutogradContext* ctx, const std::string& k) {
    ChunkedCsr c;
    c.crow = ctx->saved_data[k + "crow"].toTensor();
    c.chunk_ptr = ctx->saved_data[k + "chunk_ptr"].toTensor();
    c.chunk_begin = ctx->saved_data[k + "chunk_begin"].toTensor();
    c.chunk_row = ctx->saved_data[k + "chunk_row"].toTensor();
    c.C = ctx->saved_data[k + "chunks"].toInt();
    return c;
  }
};

inline ChunkedCsr build_chunked_csr(const Tensor& keys, int64_t rows, int64_t chunk, bool chunk_every_row,
                                    const Tensor& range_of) {
  ChunkedCsr c;
  const auto iopts = keys.options().dtype(at::kInt);
  const auto lopts = keys.options().dtype(at::kLong);
  c.chunk_begin = at::empty({0}, iopts);
  c.chunk_row = at::empty({0}, iopts);
  if (keys.numel() == 0) {
    c.crow = at::zeros({rows + 1}, iopts);
    c.chunk_ptr = at::zeros({rows + 1}, iopts);
    c.perm = at::empty({0}, lopts);
    return c;
  }
  const auto sorted = at::sort(keys, /*stable=*/true, /*dim=*/0, /*descending=*/false);
  c.perm = std::get<1>(sorted);
  const Tensor crow = at::searchsorted(std::get<0>(sorted), at::arange(rows + 1, lopts));
  c.crow = crow.to(at::kInt);
  const Tensor len = crow.narrow(0, 1, rows) - crow.narrow(0, 0, rows);
  Tensor nch = at::floor_divide(len + (chunk - 1), chunk);
  if (!chunk_every_row) nch = at::where(len > chunk, nch, at::zeros_like(len));
  const Tensor cptr = at::cat({at::zeros({1}, lopts), at::cumsum(nch, 0)});
  const auto mm = at::aminmax(range_of);
  const Tensor stats = at::stack({std::get<0>(mm).reshape({}), std::get<1>(mm).reshape({}), cptr[rows]}).cpu();
  const int64_t* s = stats.data_ptr<int64_t>();
  c.lo = s[0], c.hi = s[1], c.C = s[2];
  c.chunk_ptr = cptr.to(at::kInt);
  if (c.C > 0) {
    const Tensor row_of = at::repeat_interleave(nch, std::optional<int64_t>(c.C)); // row of each chunk
    const Tensor j = at::arange(c.C, lopts) - cptr.index_select(0, row_of);
    c.chunk_row = row_of.to(at::kInt);
    c.chunk_begin = (crow.index_select(0, row_of) + j * chunk).to(at::kInt);
  }
  return c;
}

} // namespace drtk_amd_torch
