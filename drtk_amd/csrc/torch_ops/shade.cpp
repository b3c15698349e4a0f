// drtk_amd_ext::shade -- Blinn-Phong deferred shading of an interpolated G-buffer, over drtk_amd_shade_forward /
// drtk_amd_shade_backward (include/drtk_amd.h).  No reference counterpart.  Host-only C++; the CPU key raises.
#include <array>
#include <cmath>

#include "common.hpp"

namespace {
using namespace drtk_amd_torch;
using c10::optional;

bool has(const optional<Tensor>& t) {
  return t.has_value() && t->defined();
}

// the operator's tensor arguments, in the order of its schema
enum { kNormal, kLight, kAlbedo, kAmbient, kIndex, kPos, kSpecular, kShininess, kBackground, kTensors };
using Inputs = std::array<optional<Tensor>, kTensors>;
const char* const kNames[kTensors] = {"normal_img", "light_dir", "albedo",    "ambient",   "index_img",
                                      "pos_img",    "specular",  "shininess", "background"};

struct Shape {
  int64_t N, C, H, W;
  bool albedo_is_image;
};

void check_like(const Tensor& t, const Tensor& like, const char* name) {
  TORCH_CHECK(t.layout() == at::kStrided, "shade(): expected all inputs to have torch.strided layout");
  TORCH_CHECK(
      t.device() == like.device(), "shade(): expected all inputs to be on same device, but normal_img is on ", like.device(), " and ",
      name, " on ", t.device());
}
void check_real(const Tensor& t, const Tensor& like, const char* name) {
  check_like(t, like, name);
  TORCH_CHECK(
      t.dtype() == like.dtype(), "shade(): expected ", name, " to have the type of normal_img, but normal_img has ", like.dtype(), " and ",
      name, " has ", t.dtype());
}
void check_image(const Tensor& t, const Tensor& like, const char* name, int64_t N, int64_t channels, int64_t H, int64_t W) {
  check_real(t, like, name);
  TORCH_CHECK(
      t.dim() == 4 && t.size(0) == N && t.size(1) == channels && t.size(2) == H && t.size(3) == W, "shade(): expected ", name,
      " to be [N, ", channels, ", H, W] = [", N, ", ", channels, ", ", H, ", ", W, "], but got ", name, " with sizes ", t.sizes());
}
// a parameter of `count` elements: [count] (shared by the views) or [N, count]
void check_param(const Tensor& t, const Tensor& like, const char* name, int64_t N, int64_t count) {
  check_real(t, like, name);
  TORCH_CHECK(
      (t.dim() == 1 && t.size(0) == count) || (t.dim() == 2 && t.size(0) == N && t.size(1) == count), "shade(): expected ", name,
      " to be [", count, "] or [N, ", count, "] = [", N, ", ", count, "], but got ", name, " with sizes ", t.sizes());
}

Shape shade_check(const Inputs& in, const optional<double>& gamma) {
  const Tensor& normal = *in[kNormal];
  TORCH_CHECK(
      normal.is_floating_point(), "shade(): expected normal_img to have floating point type, but normal_img has ", normal.dtype());
  TORCH_CHECK(normal.layout() == at::kStrided, "shade(): expected all inputs to have torch.strided layout");
  TORCH_CHECK(
      normal.dim() == 4 && normal.size(1) == 3, "shade(): expected normal_img to be [N, 3, H, W], but got normal_img with sizes ",
      normal.sizes());
  const Tensor& ambient = *in[kAmbient];
  TORCH_CHECK(
      ambient.dim() == 1 || ambient.dim() == 2, "shade(): expected ambient to be [C] or [N, C], but got ambient with sizes ",
      ambient.sizes());
  Shape s;
  s.N = normal.size(0), s.H = normal.size(2), s.W = normal.size(3), s.C = ambient.size(ambient.dim() - 1);
  TORCH_CHECK(s.C >= 1 && s.C <= 4, "shade(): the number of channels must be in [1, 4], but ambient has sizes ", ambient.sizes());
  TORCH_CHECK(s.H * s.W < (int64_t(1) << 31), "shade(): expected H * W to be less than 2147483648, but got H: ", s.H, ", W: ", s.W);
  check_param(ambient, normal, "ambient", s.N, s.C);
  check_param(*in[kLight], normal, "light_dir", s.N, 3);
  const Tensor& albedo = *in[kAlbedo];
  s.albedo_is_image = albedo.dim() == 4;
  if (s.albedo_is_image) check_image(albedo, normal, "albedo", s.N, s.C, s.H, s.W);
  else check_param(albedo, normal, "albedo", s.N, s.C);
  if (has(in[kIndex])) {
    const Tensor& idx = *in[kIndex];
    check_like(idx, normal, "index_img");
    TORCH_CHECK(idx.dtype() == at::kInt, "shade(): expected index_img to have int32 type, but index_img has ", idx.dtype());
    TORCH_CHECK(
        idx.dim() == 3 && idx.size(0) == s.N && idx.size(1) == s.H && idx.size(2) == s.W, "shade(): expected index_img to be [N, H, W] = [",
        s.N, ", ", s.H, ", ", s.W, "], but got index_img with sizes ", idx.sizes());
  }
  if (has(in[kSpecular])) {
    TORCH_CHECK(has(in[kPos]) && has(in[kShininess]), "shade(): specular needs pos_img and shininess");
    check_param(*in[kSpecular], normal, "specular", s.N, s.C);
    check_param(*in[kShininess], normal, "shininess", s.N, 1);
  }
  if (has(in[kPos])) check_image(*in[kPos], normal, "pos_img", s.N, 3, s.H, s.W);
  if (has(in[kBackground])) check_image(*in[kBackground], normal, "background", s.N, s.C, s.H, s.W);
  if (gamma.has_value())
    TORCH_CHECK(*gamma > 0.0 && std::isfinite(*gamma), "shade(): gamma must be positive and finite, but got ", *gamma);
  return s;
}

// What the C ABI takes: an image whose W stride is 1 is read in place, anything else is copied once; parameters are small
// and made contiguous.
struct Image {
  Tensor t;
  int64_t s[3] = {0, 0, 0};
  const void* ptr() const { return t.defined() ? t.data_ptr() : nullptr; }
};
Image image_arg(const optional<Tensor>& in) {
  Image a;
  if (!has(in)) return a;
  const int64_t d = in->dim();
  a.t = (in->size(d - 1) <= 1 || in->stride(d - 1) == 1) ? *in : in->contiguous();
  for (int64_t i = 0; i + 1 < d; ++i) a.s[i] = a.t.stride(i);
  return a;
}
struct Param {
  Tensor t;
  int64_t sN = 0;
  const void* ptr() const { return t.defined() ? t.data_ptr() : nullptr; }
};
Param param_arg(const optional<Tensor>& in) {
  Param a;
  if (!has(in)) return a;
  a.t = in->contiguous();
  a.sN = a.t.dim() == 2 ? a.t.size(1) : 0;
  return a;
}

struct Prepared {
  Image normal, pos, albedo_img, bg, index;
  Param light, albedo, ambient, specular, shininess;
  double gamma;
};
Prepared shade_prepare(const Inputs& in, const Shape& s, const optional<double>& gamma) {
  Prepared p;
  p.normal = image_arg(in[kNormal]);
  if (has(in[kSpecular])) p.pos = image_arg(in[kPos]); // (positions are read for the highlight only)
  if (s.albedo_is_image) p.albedo_img = image_arg(in[kAlbedo]);
  else p.albedo = param_arg(in[kAlbedo]);
  p.bg = image_arg(in[kBackground]);
  p.index = image_arg(in[kIndex]);
  p.light = param_arg(in[kLight]), p.ambient = param_arg(in[kAmbient]);
  if (has(in[kSpecular])) p.specular = param_arg(in[kSpecular]), p.shininess = param_arg(in[kShininess]);
  p.gamma = gamma.has_value() ? *gamma : 0.0;
  return p;
}

Tensor shade_hip(
    const Tensor& normal_img, const Tensor& light_dir, const Tensor& albedo, const Tensor& ambient, const optional<Tensor>& index_img,
    const optional<Tensor>& pos_img, const optional<Tensor>& specular, const optional<Tensor>& shininess,
    const optional<Tensor>& background, optional<double> gamma) {
  const Inputs in = {normal_img, light_dir, albedo, ambient, index_img, pos_img, specular, shininess, background};
  const Shape s = shade_check(in, gamma);
  TORCH_CHECK(normal_img.is_cuda(), "shade(): expected all inputs to be on same cuda device");
  const drtk_dtype_t dt = dtype_of(normal_img, "shade");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(normal_img.device());
  const Prepared p = shade_prepare(in, s, gamma);
  auto out = out_empty({s.N, s.C, s.H, s.W}, normal_img.options());
  check_status(
      drtk_amd_shade_forward(
          dt, p.normal.ptr(), p.normal.s, p.pos.ptr(), p.pos.s, p.albedo_img.ptr(), p.albedo_img.s, p.bg.ptr(), p.bg.s,
          static_cast<const int32_t*>(p.index.ptr()), p.index.s, p.light.ptr(), p.light.sN, p.albedo.ptr(), p.albedo.sN, p.ambient.ptr(),
          p.ambient.sN, p.specular.ptr(), p.specular.sN, p.shininess.ptr(), p.shininess.sN, p.gamma, s.N, s.C, s.H, s.W, out.data_ptr(),
          current_stream(normal_img)),
      "shade");
  return out;
}

Tensor shade_cpu(
    const Tensor& normal_img, const Tensor& light_dir, const Tensor& albedo, const Tensor& ambient, const optional<Tensor>& index_img,
    const optional<Tensor>& pos_img, const optional<Tensor>& specular, const optional<Tensor>& shininess,
    const optional<Tensor>& background, optional<double> gamma) {
  shade_check({normal_img, light_dir, albedo, ambient, index_img, pos_img, specular, shininess, background}, gamma);
  no_cpu("shade"); // a bad call reads the same with and without a device
}

Tensor shade_op(
    const Tensor& normal_img, const Tensor& light_dir, const Tensor& albedo, const Tensor& ambient, const optional<Tensor>& index_img,
    const optional<Tensor>& pos_img, const optional<Tensor>& specular, const optional<Tensor>& shininess,
    const optional<Tensor>& background, optional<double> gamma) {
  static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("drtk_amd_ext::shade", "").typed<decltype(shade_op)>();
  return op.call(normal_img, light_dir, albedo, ambient, index_img, pos_img, specular, shininess, background, gamma);
}

// The gradients of the tensors of `in` that `want` names (index_img gets none); an undefined tensor elsewhere.  A parameter's
// gradient has the parameter's shape: [K] is the sum over the views.
std::array<Tensor, kTensors> shade_backward_hip(
    const Tensor& grad_out, const Inputs& in, const optional<double>& gamma, const std::array<bool, kTensors>& want) {
  const Tensor& normal = *in[kNormal];
  const Shape s = shade_check(in, gamma);
  const drtk_dtype_t dt = dtype_of(normal, "shade_backward");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(normal.device());
  const Prepared p = shade_prepare(in, s, gamma);
  const Tensor go = grad_out.to(normal.scalar_type()).contiguous();
  const bool empty = s.N == 0 || s.H * s.W == 0;
  std::array<Tensor, kTensors> grads;
  bool params = false;
  const auto image = [&](int i) -> void* {
    if (!want[i] || !has(in[i])) return nullptr;
    grads[i] = out_empty(in[i]->sizes(), normal.options());
    return grads[i].data_ptr();
  };
  const auto param = [&](int i) -> void* {
    if (!want[i] || !has(in[i])) return nullptr;
    // (no view, or no pixel: nothing is launched, and a parameter's gradient is the empty sum)
    grads[i] = empty ? at::zeros(in[i]->sizes(), normal.options()) : out_empty(in[i]->sizes(), normal.options());
    params = true;
    return grads[i].data_ptr();
  };
  const auto sN = [&](int i) -> int64_t { return has(in[i]) && in[i]->dim() == 2 ? in[i]->size(1) : 0; };
  const bool specular = has(in[kSpecular]);
  void* g_normal = image(kNormal);
  void* g_pos = image(kPos);
  if (g_pos && !specular) grads[kPos].zero_(), g_pos = nullptr; // positions without a highlight are not used
  void* g_albedo_img = s.albedo_is_image ? image(kAlbedo) : nullptr;
  void* g_bg = image(kBackground);
  void* g_light = param(kLight);
  void* g_albedo = s.albedo_is_image ? nullptr : param(kAlbedo);
  void* g_ambient = param(kAmbient);
  void* g_specular = param(kSpecular);
  void* g_shininess = specular ? param(kShininess) : nullptr;
  if (!specular && want[kShininess] && has(in[kShininess])) grads[kShininess] = at::zeros(in[kShininess]->sizes(), normal.options());
  size_t bytes = 0;
  Tensor ws;
  if (params && !empty) {
    check_status(drtk_amd_shade_workspace_bytes(dt, s.N, s.H, s.W, &bytes), "shade_backward");
    ws = alloc_workspace(bytes, normal);
  }
  check_status(
      drtk_amd_shade_backward(
          dt, go.data_ptr(), p.normal.ptr(), p.normal.s, p.pos.ptr(), p.pos.s, p.albedo_img.ptr(), p.albedo_img.s, p.bg.ptr(), p.bg.s,
          static_cast<const int32_t*>(p.index.ptr()), p.index.s, p.light.ptr(), p.light.sN, p.albedo.ptr(), p.albedo.sN, p.ambient.ptr(),
          p.ambient.sN, p.specular.ptr(), p.specular.sN, p.shininess.ptr(), p.shininess.sN, p.gamma, s.N, s.C, s.H, s.W, g_normal, g_pos,
          g_albedo_img, g_bg, g_light, sN(kLight), g_albedo, sN(kAlbedo), g_ambient, sN(kAmbient), g_specular, sN(kSpecular), g_shininess,
          sN(kShininess), ws.defined() ? ws.data_ptr() : nullptr, bytes, current_stream(normal)),
      "shade_backward");
  return grads;
}

class ShadeFunction : public torch::autograd::Function<ShadeFunction> {
 public:
  static Tensor forward(
      AutogradContext* ctx, const Tensor& normal_img, const Tensor& light_dir, const Tensor& albedo, const Tensor& ambient,
      const optional<Tensor>& index_img, const optional<Tensor>& pos_img, const optional<Tensor>& specular,
      const optional<Tensor>& shininess, const optional<Tensor>& background, optional<double> gamma) {
    const Inputs in = {normal_img, light_dir, albedo, ambient, index_img, pos_img, specular, shininess, background};
    int64_t present = 0, wanted = 0;
    tensor_list saved; // nothing but the inputs: the backward recomputes the shading
    for (int i = 0; i < kTensors; ++i) {
      if (!has(in[i])) continue;
      present |= int64_t(1) << i;
      if (in[i]->is_floating_point() && in[i]->requires_grad()) wanted |= int64_t(1) << i;
      saved.push_back(*in[i]);
    }
    ctx->saved_data["data"] = std::make_tuple(present, wanted, gamma.has_value(), gamma.has_value() ? *gamma : 0.0);
    Tensor out;
    {
      at::AutoDispatchBelowADInplaceOrView g;
      out = shade_op(normal_img, light_dir, albedo, ambient, index_img, pos_img, specular, shininess, background, gamma);
    }
    ctx->save_for_backward(saved);
    return out;
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grad_outputs) {
    int64_t present, wanted;
    bool has_gamma;
    double gamma_value;
    std::tie(present, wanted, has_gamma, gamma_value) = ctx->saved_data["data"].to<std::tuple<int64_t, int64_t, bool, double>>();
    tensor_list grads(kTensors + 1); // gamma gets none
    if (!wanted || !grad_outputs[0].defined()) return grads;
    // the backward is a kernel, not a graph of differentiable operations: with create_graph=True its result would pass for a constant
    TORCH_CHECK(
        !at::GradMode::is_enabled(), "shade(): double backward (create_graph=True) is not supported by drtk_amd's shade kernels");
    const auto saved = ctx->get_saved_variables();
    Inputs in;
    std::array<bool, kTensors> want;
    size_t at = 0;
    for (int i = 0; i < kTensors; ++i) {
      if ((present >> i) & 1) in[i] = saved[at++];
      want[i] = (wanted >> i) & 1;
    }
    const auto g = shade_backward_hip(grad_outputs[0], in, has_gamma ? optional<double>(gamma_value) : optional<double>(), want);
    for (int i = 0; i < kTensors; ++i) {
      if (want[i]) grads[i] = g[i];
    }
    return grads;
  }
};

Tensor shade_autograd(
    const Tensor& normal_img, const Tensor& light_dir, const Tensor& albedo, const Tensor& ambient, const optional<Tensor>& index_img,
    const optional<Tensor>& pos_img, const optional<Tensor>& specular, const optional<Tensor>& shininess,
    const optional<Tensor>& background, optional<double> gamma) {
  return ShadeFunction::apply(normal_img, light_dir, albedo, ambient, index_img, pos_img, specular, shininess, background, gamma);
}

optional<Tensor> to_float(const optional<Tensor>& t) {
  return has(t) ? optional<Tensor>(at::autocast::cached_cast(at::kFloat, *t)) : t;
}

Tensor shade_autocast(
    const Tensor& normal_img, const Tensor& light_dir, const Tensor& albedo, const Tensor& ambient, const optional<Tensor>& index_img,
    const optional<Tensor>& pos_img, const optional<Tensor>& specular, const optional<Tensor>& shininess,
    const optional<Tensor>& background, optional<double> gamma) {
  c10::impl::ExcludeDispatchKeyGuard no_autocast(c10::DispatchKey::Autocast);
  const auto f = [](const Tensor& t) { return at::autocast::cached_cast(at::kFloat, t); };
  return shade_op(
      f(normal_img), f(light_dir), f(albedo), f(ambient), index_img, to_float(pos_img), to_float(specular), to_float(shininess),
      to_float(background), gamma);
}

} // namespace

TORCH_LIBRARY_FRAGMENT(drtk_amd_ext, m) {
  m.def(
      "shade(Tensor normal_img, Tensor light_dir, Tensor albedo, Tensor ambient, Tensor? index_img, Tensor? pos_img, Tensor? specular, "
      "Tensor? shininess, Tensor? background, float? gamma) -> Tensor");
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, Autograd, m) {
  m.impl("shade", &shade_autograd);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, Autocast, m) {
  m.impl("shade", shade_autocast);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CUDA, m) {
  m.impl("shade", &shade_hip);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CPU, m) {
  m.impl("shade", &shade_cpu);
}
