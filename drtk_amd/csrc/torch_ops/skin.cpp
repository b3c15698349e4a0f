// drtk_amd_ext::skin -- linear blend skinning over drtk_amd_skin_* (csrc/skin.hip): the posed vertices and the gradients
// to the rest pose, the weights and the joint transforms, without float atomics.  The gradient to the transforms is a
// many-to-few reduction through the JOINT INCIDENCE of joint_idx (CSR over joints, every row chunked), built here with
// ATen where joint_idx lives and cached under geometry.cpp's key rule (tensor identity + version counter, pinned, LRU).
#include "common.hpp"

#include <hip/hip_runtime_api.h>

namespace {
using namespace drtk_amd_torch;

constexpr int64_t kChunk = DRTK_SKIN_CHUNK;

struct JointIncidence {
  Tensor idx32; // int32 [V,K] contiguous
  Tensor crow, entries; // int32 [J+1], [V*K] (the first crow[J] are entries; the rest are the empty slots)
  Tensor chunk_ptr, chunk_begin, chunk_joint; // int32 [J+1], [C], [C]
  int64_t V = 0, K = 0, J = 0, C = 0;
};

// Stable sort of the slots' joints (empty slots keyed J, so they sort behind every joint): the permutation is then
// ascending in i*K+k within a joint; searchsorted gives the row starts.  One host read per build: the index range (an index
// outside [-1, J) would make the kernels read out of bounds) and the number of chunks (a launch size).
JointIncidence build_joint_incidence(const Tensor& t, int64_t J, const char* op) {
  JointIncidence inc;
  inc.V = t.size(0), inc.K = t.size(1), inc.J = J;
  const int64_t E = inc.V * inc.K;
  TORCH_CHECK(J >= 0 && J < (int64_t(1) << 27) && E < (int64_t(1) << 31), op, "(): mesh too large for int32 joint incidence");
  const auto iopts = t.options().dtype(at::kInt);
  const auto lopts = t.options().dtype(at::kLong);
  inc.idx32 = t.detach().to(at::kInt).contiguous();
  inc.chunk_begin = at::empty({0}, iopts);
  inc.chunk_joint = at::empty({0}, iopts);
  if (E == 0) {
    inc.crow = at::zeros({J + 1}, iopts);
    inc.entries = at::empty({0}, iopts);
    inc.chunk_ptr = at::zeros({J + 1}, iopts);
    return inc;
  }
  const Tensor tl = t.detach().to(at::kLong).contiguous().reshape({-1});
  const Tensor keys = at::where(tl < 0, at::full_like(tl, J), tl);
  const auto sorted = at::sort(keys, /*stable=*/true, /*dim=*/0, /*descending=*/false);
  inc.entries = std::get<1>(sorted).to(at::kInt);
  const Tensor crow = at::searchsorted(std::get<0>(sorted), at::arange(J + 1, lopts));
  inc.crow = crow.to(at::kInt);
  const Tensor len = crow.narrow(0, 1, J) - crow.narrow(0, 0, J);
  const Tensor nch = at::floor_divide(len + (kChunk - 1), kChunk); // every row is chunked
  const Tensor cptr = at::cat({at::zeros({1}, lopts), at::cumsum(nch, 0)});
  const auto mm = at::aminmax(tl);
  const Tensor stats = at::stack({std::get<0>(mm).reshape({}), std::get<1>(mm).reshape({}), cptr[J]}).cpu();
  const int64_t* s = stats.data_ptr<int64_t>();
  TORCH_CHECK(s[0] >= -1 && s[1] < J, op, "(): joint_idx contains a joint index outside [-1, ", J, ")");
  inc.C = s[2];
  inc.chunk_ptr = cptr.to(at::kInt);
  if (inc.C > 0) {
    const Tensor rows = at::repeat_interleave(nch, std::optional<int64_t>(inc.C)); // joint of each chunk
    const Tensor j = at::arange(inc.C, lopts) - cptr.index_select(0, rows);
    inc.chunk_joint = rows.to(at::kInt);
    inc.chunk_begin = (crow.index_select(0, rows) + j * kChunk).to(at::kInt);
  }
  return inc;
}

// The cache of geometry.cpp's vertex incidence, for [V,K] index tensors: identity + version of the tensor, no content
// hashing; an in-place edit bumps the version counter and misses; each entry pins its tensor so that a recycled allocation
// cannot alias a stale entry; 128 entries, LRU.
using JointKey = std::array<int64_t, 12>;
struct JointKeyHash {
  size_t operator()(const JointKey& k) const {
    uint64_t h = 1469598103934665603ull; // FNV-1a over the fields
    for (int64_t x : k) {
      h ^= static_cast<uint64_t>(x);
      h *= 1099511628211ull;
    }
    return static_cast<size_t>(h);
  }
};
JointKey joint_key(const Tensor& t, int64_t J) {
  return {static_cast<int64_t>(t.device().type()),
          static_cast<int64_t>(t.device().index()),
          static_cast<int64_t>(reinterpret_cast<uintptr_t>(t.storage().unsafeGetStorageImpl())),
          static_cast<int64_t>(reinterpret_cast<uintptr_t>(t.data_ptr())),
          t.size(0),
          t.size(1),
          t.stride(0),
          t.stride(1),
          t.storage_offset(),
          static_cast<int64_t>(t.scalar_type()),
          J,
          static_cast<int64_t>(t.unsafeGetTensorImpl()->version_counter().current_version())};
}

class JointIncidenceCache {
 public:
  static constexpr size_t kCapacity = 128;
  static JointIncidenceCache& instance() {
    static JointIncidenceCache c;
    return c;
  }
  JointIncidence get(const Tensor& idx, int64_t J, const char* op) {
    const JointKey key = joint_key(idx, J);
    {
      std::lock_guard<std::mutex> lock(mu_);
      if (const JointIncidence* hit = touch(key)) {
        ++hits_;
        return *hit;
      }
    }
    if (idx.is_cuda()) {
      // the build reads three numbers back and allocates: not capturable
      hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
      const hipStream_t s = c10::hip::getCurrentHIPStream(idx.device().index()).stream();
      TORCH_CHECK(hipStreamIsCapturing(s, &st) != hipSuccess || st == hipStreamCaptureStatusNone, op,
                  "(): the joint incidence of this index tensor is not cached yet, and it cannot be built while the "
                  "stream is being captured -- run the op once with the same joint_idx before the capture");
    }
    JointIncidence built = build_joint_incidence(idx, J, op);
    std::lock_guard<std::mutex> lock(mu_);
    if (const JointIncidence* hit = touch(key)) return *hit;
    ++misses_;
    while (lru_.size() >= kCapacity) {
      index_.erase(lru_.back().key);
      lru_.pop_back();
    }
    lru_.push_front(Entry{key, idx, built});
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
    JointKey key;
    Tensor pinned_idx;
    JointIncidence inc;
  };
  const JointIncidence* touch(const JointKey& key) {
    const auto it = index_.find(key);
    if (it == index_.end()) return nullptr;
    lru_.splice(lru_.begin(), lru_, it->second);
    return &it->second->inc;
  }
  std::mutex mu_;
  std::list<Entry> lru_;
  std::unordered_map<JointKey, std::list<Entry>::iterator, JointKeyHash> index_;
  int64_t hits_ = 0, misses_ = 0;
};

JointIncidence joint_incidence_of(const Tensor& idx, int64_t J, const char* op) {
  TORCH_CHECK(idx.defined() && idx.layout() == at::kStrided, op, "(): expected joint_idx to be a strided tensor");
  TORCH_CHECK(idx.scalar_type() == at::kInt || idx.scalar_type() == at::kLong, op,
              "(): expected joint_idx to be int32 or int64, got ", idx.scalar_type());
  TORCH_CHECK(idx.dim() == 2, op, "(): expected joint_idx of shape [V, K]");
  TORCH_CHECK(idx.size(1) >= 1 && idx.size(1) <= DRTK_SKIN_MAX_SLOTS, op, "(): expected 1 <= K <= ", DRTK_SKIN_MAX_SLOTS,
              " slots per vertex, got K = ", idx.size(1));
  return JointIncidenceCache::instance().get(idx, J, op);
}

// What the kernels read.  v: one row [V,3] (v_sN = 0) or N of them; transforms: read in place where rows 0..2 of a joint
// are 12 consecutive elements (a [..., :3, :] view of a 4x4 tensor is), copied otherwise.
struct SkinArgs {
  Tensor v, w, t;
  JointIncidence inc;
  int64_t N = 0, V = 0, J = 0, K = 0, v_sN = 0, t_sN = 0, t_sJ = 12;
};
SkinArgs skin_prep(const Tensor& v_, const Tensor& idx, const Tensor& w_, const Tensor& t_) {
  const char* op = "skin";
  SkinArgs a;
  TORCH_CHECK(v_.is_cuda(), op, "(): drtk_amd implements the MI355X (HIP) path only; got CPU tensors");
  dtype_of(v_, op);
  TORCH_CHECK((v_.dim() == 2 || v_.dim() == 3) && v_.size(-1) == 3, op, "(): expected v of shape [N, V, 3], [1, V, 3] or [V, 3]");
  TORCH_CHECK(t_.dim() == 4 && (t_.size(2) == 3 || t_.size(2) == 4) && t_.size(3) == 4, op,
              "(): expected transforms of shape [N, J, 3, 4] or [N, J, 4, 4]");
  TORCH_CHECK(t_.device() == v_.device() && w_.device() == v_.device() && idx.device() == v_.device(), op,
              "(): expected joint_idx, joint_weights and transforms on the device of v");
  TORCH_CHECK(t_.scalar_type() == v_.scalar_type() && w_.scalar_type() == v_.scalar_type(), op,
              "(): expected joint_weights and transforms to have the dtype of v, got ", w_.scalar_type(), " and ",
              t_.scalar_type(), " for ", v_.scalar_type());
  a.N = t_.size(0), a.J = t_.size(1);
  Tensor v = v_.dim() == 2 ? v_.unsqueeze(0) : v_;
  a.V = v.size(1);
  TORCH_CHECK(v.size(0) == 1 || v.size(0) == a.N, op, "(): expected the batch size of v to be 1 or ", a.N, ", got ", v.size(0));
  if (v.size(0) > 1 && v.stride(0) == 0) v = v.narrow(0, 0, 1); // a stride-0 expand is read as one row
  a.v = v.contiguous();
  a.v_sN = a.v.size(0) == 1 ? 0 : a.V * 3;
  a.inc = joint_incidence_of(idx, a.J, op);
  a.K = a.inc.K;
  TORCH_CHECK(a.inc.V == a.V, op, "(): expected joint_idx of shape [V, K] with V = ", a.V, ", got ", a.inc.V);
  TORCH_CHECK(w_.dim() == 2 && w_.size(0) == a.V && w_.size(1) == a.K, op, "(): expected joint_weights of the shape of joint_idx");
  a.w = w_.contiguous();
  const bool in_place = t_.stride(3) == 1 && t_.stride(2) == 4 && (a.J <= 1 || t_.stride(1) >= 12) &&
                        (a.N <= 1 || t_.stride(0) == 0 || t_.stride(0) >= (a.J - 1) * (a.J > 1 ? t_.stride(1) : 0) + 12);
  a.t = in_place ? t_ : t_.contiguous();
  a.t_sJ = a.J > 1 ? a.t.stride(1) : 12;
  a.t_sN = a.N > 1 ? a.t.stride(0) : 0;
  return a;
}

Tensor skin_apply(const SkinArgs& a) {
  auto out = out_empty({a.N, a.V, 3}, a.v.options());
  check_status(drtk_amd_skin_forward(dtype_of(a.v, "skin"), a.v.data_ptr(), a.v_sN, a.inc.idx32.data_ptr<int32_t>(),
                                     a.w.data_ptr(), a.t.data_ptr(), a.t_sN, a.t_sJ, a.N, a.V, a.J, a.K, out.data_ptr(),
                                     current_stream(a.v)),
               "skin");
  return out;
}

Tensor skin_hip(const Tensor& v, const Tensor& idx, const Tensor& w, const Tensor& t) {
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
  return skin_apply(skin_prep(v, idx, w, t));
}

class SkinFunction : public torch::autograd::Function<SkinFunction> {
 public:
  static tensor_list forward(AutogradContext* ctx, const Tensor& v, const Tensor& idx, const Tensor& w, const Tensor& t) {
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
    ctx->set_materialize_grads(false);
    const SkinArgs a = skin_prep(v, idx, w, t);
    ctx->save_for_backward({a.v, a.w, a.t});
    // decided on the inputs as passed: the copies the kernels read never require grad
    ctx->saved_data["need"] = std::vector<int64_t>{v.requires_grad(), w.requires_grad(), t.requires_grad()};
    ctx->saved_data["v_sizes"] = v.sizes().vec();
    ctx->saved_data["t_rows"] = t.size(2);
    ctx->saved_data["strides"] = std::vector<int64_t>{a.N, a.V, a.J, a.K, a.v_sN, a.t_sN, a.t_sJ, a.inc.C};
    ctx->saved_data["idx"] = a.inc.idx32;
    ctx->saved_data["crow"] = a.inc.crow;
    ctx->saved_data["entries"] = a.inc.entries;
    ctx->saved_data["chunk_ptr"] = a.inc.chunk_ptr;
    ctx->saved_data["chunk_begin"] = a.inc.chunk_begin;
    ctx->saved_data["chunk_joint"] = a.inc.chunk_joint;
    at::AutoDispatchBelowADInplaceOrView g;
    return {skin_apply(a)};
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list go) {
    const auto need = ctx->saved_data["need"].toIntVector();
    if (!go[0].defined() || !(need[0] || need[1] || need[2])) return {Tensor(), Tensor(), Tensor(), Tensor()};
    // the backward passes are kernels, not differentiable graphs: their second-order terms would be silently zero
    TORCH_CHECK(!at::GradMode::is_enabled(), "skin_backward(): double backward (create_graph=True) is not supported by "
                "drtk_amd's skinning kernels; the PyTorch formulation (CPU tensors) supports it");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(go[0].device());
    const auto saved = ctx->get_saved_variables();
    const Tensor &v = saved[0], &w = saved[1], &t = saved[2];
    const auto s = ctx->saved_data["strides"].toIntVector();
    const int64_t N = s[0], V = s[1], J = s[2], K = s[3], v_sN = s[4], t_sN = s[5], t_sJ = s[6], C = s[7];
    const Tensor g = go[0].contiguous(); // dtype of v, in which the forward ran
    const auto v_sizes = ctx->saved_data["v_sizes"].toIntVector();
    const int64_t gv_B = v_sizes.size() == 3 ? v_sizes[0] : 1;
    const int64_t rows = ctx->saved_data["t_rows"].toInt();
    Tensor gv, gw, gt, ws;
    if (need[0]) gv = out_empty({gv_B, V, 3}, g.options());
    if (need[1]) gw = out_empty({V, K}, g.options());
    size_t bytes = 0;
    const drtk_dtype_t dt = dtype_of(g, "skin_backward");
    if (need[2]) {
      gt = out_empty({N, J, rows, 4}, g.options());
      check_status(drtk_amd_skin_backward_workspace_bytes(dt, N, C, &bytes), "skin_backward");
      if (bytes) ws = alloc_workspace(bytes, g);
    }
    auto iptr = [&](const char* k) { return ctx->saved_data[k].toTensor().data_ptr<int32_t>(); };
    check_status(
        drtk_amd_skin_backward(
            dt, g.data_ptr(), v.data_ptr(), v_sN, iptr("idx"), w.data_ptr(), t.data_ptr(), t_sN, t_sJ, iptr("crow"),
            iptr("entries"), iptr("chunk_ptr"), iptr("chunk_begin"), iptr("chunk_joint"), C, N, V, J, K, gv_B,
            gv.defined() ? gv.data_ptr() : nullptr, gw.defined() ? gw.data_ptr() : nullptr, rows,
            gt.defined() ? gt.data_ptr() : nullptr, ws.defined() ? ws.data_ptr() : nullptr, bytes, current_stream(g)),
        "skin_backward");
    if (gv.defined()) gv = gv.view(v_sizes);
    return {gv, Tensor(), gw, gt};
  }
};
Tensor skin_autograd(const Tensor& v, const Tensor& idx, const Tensor& w, const Tensor& t) {
  return SkinFunction::apply(v, idx, w, t)[0];
}
Tensor skin_cpu(const Tensor&, const Tensor&, const Tensor&, const Tensor&) {
  no_cpu("skin");
}

std::tuple<Tensor, Tensor> joint_incidence(const Tensor& idx, int64_t num_joints) {
  const JointIncidence inc = joint_incidence_of(idx, num_joints, "joint_incidence");
  return {inc.crow, inc.entries};
}
std::vector<int64_t> skin_cache_stats() {
  return JointIncidenceCache::instance().stats();
}
void skin_cache_clear() {
  JointIncidenceCache::instance().clear();
}

} // namespace

TORCH_LIBRARY_FRAGMENT(drtk_amd_ext, m) {
  m.def("skin(Tensor v, Tensor joint_idx, Tensor joint_weights, Tensor transforms) -> Tensor");
  m.def("joint_incidence(Tensor joint_idx, int num_joints) -> (Tensor, Tensor)", &joint_incidence);
  m.def("skin_cache_stats() -> int[]", &skin_cache_stats);
  m.def("skin_cache_clear() -> ()", &skin_cache_clear);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, Autograd, m) {
  m.impl("skin", &skin_autograd);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CUDA, m) {
  m.impl("skin", &skin_hip);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CPU, m) {
  m.impl("skin", &skin_cpu);
}
