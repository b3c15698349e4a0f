// drtk_amd_ext::ssim / ssim_map / photometric_loss -- the fused image losses, over drtk_amd_image_loss_forward /
// drtk_amd_image_loss_backward (include/drtk_amd.h).  No reference counterpart.  Host-only C++; the CPU key raises.
#include <cmath>

#include "common.hpp"

namespace {
using namespace drtk_amd_torch;

enum { IL_MAP = 0, IL_SSIM = 1, IL_PHOTOMETRIC = 2 };
const char* const kNames[3] = {"ssim", "ssim", "photometric_loss"};

struct LossParams {
  int64_t mode, window_size;
  double sigma, data_range, l1_weight, ssim_weight;
  bool valid;
};

void loss_check(const Tensor& img, const Tensor& target, const c10::optional<Tensor>& weight, const LossParams& p) {
  const char* op = kNames[p.mode];
  TORCH_CHECK(img.defined() && target.defined(), op, "(): expected img and target to be defined");
  TORCH_CHECK(img.dim() == 4, op, "(): expected img.ndim == 4 ([N, C, H, W]), but got img with sizes ", img.sizes());
  TORCH_CHECK(
      img.sizes() == target.sizes(), op, "(): expected img and target to have the same sizes, but got ", img.sizes(), " and ",
      target.sizes());
  TORCH_CHECK(
      img.scalar_type() == target.scalar_type(), op, "(): expected img and target to have the same dtype, but got ", img.dtype(),
      " and ", target.dtype());
  TORCH_CHECK(img.device() == target.device(), op, "(): expected img and target to be on the same device");
  dtype_of(img, op); // float32 and float64 only
  const int64_t N = img.size(0), C = img.size(1), H = img.size(2), W = img.size(3);
  TORCH_CHECK(N >= 1 && C >= 1 && H >= 1 && W >= 1, op, "(): expected non-empty images, but got img with sizes ", img.sizes());
  TORCH_CHECK(H * W < (int64_t(1) << 31), op, "(): expected H * W to be less than 2147483648, but got H: ", H, ", W: ", W);
  TORCH_CHECK_VALUE(
      p.window_size >= 3 && p.window_size <= 15 && p.window_size % 2 == 1, op, "(): window_size must be odd and in [3, 15], but got ",
      p.window_size);
  TORCH_CHECK_VALUE(p.sigma > 0.0 && std::isfinite(p.sigma), op, "(): sigma must be positive and finite, but got ", p.sigma);
  TORCH_CHECK_VALUE(
      p.data_range > 0.0 && std::isfinite(p.data_range), op, "(): data_range must be positive and finite, but got ", p.data_range);
  TORCH_CHECK_VALUE(
      !p.valid || (H >= p.window_size && W >= p.window_size), op, "(): padding=\"valid\" needs H, W >= window_size (", p.window_size,
      "), but got H: ", H, ", W: ", W);
  if (weight.has_value() && weight->defined()) {
    const Tensor& w = *weight;
    TORCH_CHECK(p.mode != IL_MAP, op, "(): reduction=\"none\" takes no weight");
    const bool shape_ok = (w.dim() == 3 && w.sizes() == at::IntArrayRef({N, H, W})) || (w.dim() == 4 && w.sizes() == at::IntArrayRef({N, 1, H, W}));
    TORCH_CHECK(shape_ok, op, "(): expected weight to be [N, H, W] or [N, 1, H, W] = [", N, ", ", H, ", ", W, "], but got ", w.sizes());
    TORCH_CHECK(
        w.scalar_type() == at::kBool || w.scalar_type() == img.scalar_type(), op, "(): expected weight to be bool or ", img.dtype(),
        ", but got ", w.dtype());
    TORCH_CHECK(w.device() == img.device(), op, "(): expected weight to be on the images' device");
  }
}

// rows contiguous: read in place whatever the view / channel / row strides (channel slices of an RGBA render, view slices)
Tensor rows(const Tensor& t) {
  return (t.size(3) <= 1 || t.stride(3) == 1) ? t : t.contiguous();
}

struct WeightArg {
  Tensor t;
  int kind = 0;
  int64_t strides[2] = {0, 0};
};
WeightArg prep_weight(const c10::optional<Tensor>& weight) {
  WeightArg a;
  if (!weight.has_value() || !weight->defined()) return a;
  Tensor w = weight->detach();
  if (w.dim() == 4) w = w.select(1, 0);
  if (w.size(2) > 1 && w.stride(2) != 1) w = w.contiguous();
  a.t = w, a.kind = w.scalar_type() == at::kBool ? 1 : 2;
  a.strides[0] = w.stride(0), a.strides[1] = w.stride(1);
  return a;
}

struct LossResult {
  Tensor out, maps, scalars;
};

LossResult loss_forward_hip(const Tensor& img, const Tensor& target, const c10::optional<Tensor>& weight, const LossParams& p, bool with_maps) {
  const char* op = kNames[p.mode];
  loss_check(img, target, weight, p);
  if (!img.is_cuda()) no_cpu(op);
  const drtk_dtype_t dt = dtype_of(img, op);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(img.device());
  const Tensor x = rows(img), y = rows(target);
  const WeightArg w = prep_weight(weight);
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t off = p.valid ? p.window_size / 2 : 0, OH = H - 2 * off, OW = W - 2 * off;
  const int64_t xs[3] = {x.stride(0), x.stride(1), x.stride(2)}, ys[3] = {y.stride(0), y.stride(1), y.stride(2)};
  LossResult r;
  r.out = p.mode == IL_MAP ? out_empty({N, C, OH, OW}, x.options()) : out_empty({}, x.options());
  if (with_maps) r.maps = out_empty({3, N, C, OH, OW}, x.options());
  size_t bytes = 0;
  Tensor ws;
  if (p.mode != IL_MAP) {
    check_status(drtk_amd_image_loss_workspace_bytes(N, H, W, static_cast<int>(p.window_size), p.valid, &bytes), op);
    r.scalars = out_empty({4}, x.options().dtype(at::kDouble));
    ws = out_empty({static_cast<int64_t>(bytes / sizeof(double))}, x.options().dtype(at::kDouble));
  }
  check_status(
      drtk_amd_image_loss_forward(
          dt, x.data_ptr(), xs, y.data_ptr(), ys, w.kind ? w.t.data_ptr() : nullptr, w.kind, w.strides, N, C, H, W,
          static_cast<int>(p.window_size), p.sigma, p.data_range, p.valid, static_cast<int>(p.mode), p.l1_weight, p.ssim_weight,
          r.out.data_ptr(), with_maps ? r.maps.data_ptr() : nullptr, r.scalars.defined() ? r.scalars.data_ptr() : nullptr,
          ws.defined() ? ws.data_ptr() : nullptr, bytes, current_stream(x)),
      op);
  return r;
}

Tensor loss_backward_hip(
    const Tensor& img, const Tensor& target, const c10::optional<Tensor>& weight, const LossParams& p, const Tensor& maps,
    const Tensor& scalars, const Tensor& grad_out) {
  const char* op = kNames[p.mode];
  const drtk_dtype_t dt = dtype_of(img, op);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(img.device());
  const Tensor x = rows(img), y = rows(target);
  const WeightArg w = prep_weight(weight);
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t xs[3] = {x.stride(0), x.stride(1), x.stride(2)}, ys[3] = {y.stride(0), y.stride(1), y.stride(2)};
  const Tensor g = grad_out.to(x.scalar_type()).contiguous(); // (an expanded scalar gradient becomes one element)
  TORCH_CHECK(g.numel() == (p.mode == IL_MAP ? maps.numel() / 3 : 1), op, "(): the gradient has sizes ", grad_out.sizes());
  Tensor grad_img = out_empty({N, C, H, W}, x.options());
  check_status(
      drtk_amd_image_loss_backward(
          dt, x.data_ptr(), xs, y.data_ptr(), ys, w.kind ? w.t.data_ptr() : nullptr, w.kind, w.strides, N, C, H, W,
          static_cast<int>(p.window_size), p.sigma, p.data_range, p.valid, static_cast<int>(p.mode), p.l1_weight, p.ssim_weight,
          maps.data_ptr(), g.data_ptr(), scalars.defined() ? scalars.data_ptr() : nullptr, grad_img.data_ptr(), current_stream(x)),
      op);
  return grad_img;
}

// img gets a gradient; target and weight get none.  Saved: the two images, the weight, the three maps and the scalars.
class ImageLossFunction : public torch::autograd::Function<ImageLossFunction> {
 public:
  static Tensor forward(
      AutogradContext* ctx, const Tensor& img, const Tensor& target, const c10::optional<Tensor>& weight, int64_t mode,
      int64_t window_size, double sigma, double data_range, bool valid, double l1_weight, double ssim_weight) {
    const LossParams p = {mode, window_size, sigma, data_range, l1_weight, ssim_weight, valid};
    at::AutoDispatchBelowADInplaceOrView g;
    const LossResult r = loss_forward_hip(img, target, weight, p, true);
    const bool has_w = weight.has_value() && weight->defined();
    ctx->save_for_backward({img, target, has_w ? weight->detach() : Tensor(), r.maps, r.scalars});
    ctx->saved_data["mode"] = mode, ctx->saved_data["window_size"] = window_size, ctx->saved_data["sigma"] = sigma;
    ctx->saved_data["data_range"] = data_range, ctx->saved_data["valid"] = valid, ctx->saved_data["l1_weight"] = l1_weight;
    ctx->saved_data["ssim_weight"] = ssim_weight;
    return r.out;
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grad_outputs) {
    tensor_list grads(10);
    if (!grad_outputs[0].defined()) return grads;
    const LossParams p = {
        ctx->saved_data["mode"].toInt(),        ctx->saved_data["window_size"].toInt(),  ctx->saved_data["sigma"].toDouble(),
        ctx->saved_data["data_range"].toDouble(), ctx->saved_data["l1_weight"].toDouble(), ctx->saved_data["ssim_weight"].toDouble(),
        ctx->saved_data["valid"].toBool()};
    // the backward is a kernel, not a graph of differentiable operations: with create_graph=True its result would pass for a constant
    TORCH_CHECK(
        !at::GradMode::is_enabled(), kNames[p.mode],
        "(): double backward (create_graph=True) is not supported by drtk_amd's image-loss kernels");
    const auto saved = ctx->get_saved_variables();
    const c10::optional<Tensor> weight = saved[2].defined() ? c10::optional<Tensor>(saved[2]) : c10::nullopt;
    grads[0] = loss_backward_hip(saved[0], saved[1], weight, p, saved[3], saved[4], grad_outputs[0]);
    return grads;
  }
};

Tensor loss_autograd(const Tensor& img, const Tensor& target, const c10::optional<Tensor>& weight, const LossParams& p) {
  loss_check(img, target, weight, p);
  TORCH_CHECK(
      !(at::GradMode::is_enabled() && target.requires_grad()), kNames[p.mode],
      "(): target requires a gradient, and only img gets one.  The loss is symmetric in its two images: pass target.detach() here "
      "and, for the gradient of target, call again with the arguments exchanged, ",
      kNames[p.mode], "(target, img.detach(), ...)");
  if (at::GradMode::is_enabled() && img.requires_grad())
    return ImageLossFunction::apply(img, target, weight, p.mode, p.window_size, p.sigma, p.data_range, p.valid, p.l1_weight, p.ssim_weight);
  at::AutoDispatchBelowADInplaceOrView g;
  return loss_forward_hip(img, target, weight, p, false).out; // nothing but the partial sums and the scalars is written
}

Tensor autocast_image(const Tensor& t) {
  return at::autocast::cached_cast(at::kFloat, t);
}
c10::optional<Tensor> autocast_weight(const c10::optional<Tensor>& w) {
  if (!w.has_value() || !w->defined() || w->scalar_type() == at::kBool) return w;
  return c10::optional<Tensor>(at::autocast::cached_cast(at::kFloat, *w));
}

// ---- the three operators, one function per dispatch key -------------------------------------------------------------
#define SSIM_ARGS const Tensor &img, const Tensor &target, const c10::optional<Tensor>&weight, int64_t window_size, double sigma, double data_range, bool valid
#define SSIM_PARAMS(mode) LossParams{mode, window_size, sigma, data_range, 0.0, 0.0, valid}
#define MAP_ARGS const Tensor &img, const Tensor &target, int64_t window_size, double sigma, double data_range, bool valid
#define PHOTO_ARGS const Tensor &img, const Tensor &target, const c10::optional<Tensor>&weight, double l1_weight, double ssim_weight, int64_t window_size, double sigma, double data_range, bool valid
#define PHOTO_PARAMS LossParams{IL_PHOTOMETRIC, window_size, sigma, data_range, l1_weight, ssim_weight, valid}

Tensor ssim_hip(SSIM_ARGS) { return loss_forward_hip(img, target, weight, SSIM_PARAMS(IL_SSIM), false).out; }
Tensor ssim_map_hip(MAP_ARGS) { return loss_forward_hip(img, target, c10::nullopt, SSIM_PARAMS(IL_MAP), false).out; }
Tensor photometric_hip(PHOTO_ARGS) { return loss_forward_hip(img, target, weight, PHOTO_PARAMS, false).out; }

Tensor ssim_cpu(SSIM_ARGS) {
  loss_check(img, target, weight, SSIM_PARAMS(IL_SSIM)); // a bad call reads the same with and without a device
  no_cpu("ssim");
}
Tensor ssim_map_cpu(MAP_ARGS) {
  loss_check(img, target, c10::nullopt, SSIM_PARAMS(IL_MAP));
  no_cpu("ssim");
}
Tensor photometric_cpu(PHOTO_ARGS) {
  loss_check(img, target, weight, PHOTO_PARAMS);
  no_cpu("photometric_loss");
}

Tensor ssim_autograd(SSIM_ARGS) { return loss_autograd(img, target, weight, SSIM_PARAMS(IL_SSIM)); }
Tensor ssim_map_autograd(MAP_ARGS) { return loss_autograd(img, target, c10::nullopt, SSIM_PARAMS(IL_MAP)); }
Tensor photometric_autograd(PHOTO_ARGS) { return loss_autograd(img, target, weight, PHOTO_PARAMS); }

Tensor ssim_op(SSIM_ARGS) {
  static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("drtk_amd_ext::ssim", "").typed<decltype(ssim_op)>();
  return op.call(img, target, weight, window_size, sigma, data_range, valid);
}
Tensor ssim_map_op(MAP_ARGS) {
  static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("drtk_amd_ext::ssim_map", "").typed<decltype(ssim_map_op)>();
  return op.call(img, target, window_size, sigma, data_range, valid);
}
Tensor photometric_op(PHOTO_ARGS) {
  static auto op =
      c10::Dispatcher::singleton().findSchemaOrThrow("drtk_amd_ext::photometric_loss", "").typed<decltype(photometric_op)>();
  return op.call(img, target, weight, l1_weight, ssim_weight, window_size, sigma, data_range, valid);
}

Tensor ssim_autocast(SSIM_ARGS) {
  c10::impl::ExcludeDispatchKeyGuard no_autocast(c10::DispatchKey::Autocast);
  return ssim_op(autocast_image(img), autocast_image(target), autocast_weight(weight), window_size, sigma, data_range, valid);
}
Tensor ssim_map_autocast(MAP_ARGS) {
  c10::impl::ExcludeDispatchKeyGuard no_autocast(c10::DispatchKey::Autocast);
  return ssim_map_op(autocast_image(img), autocast_image(target), window_size, sigma, data_range, valid);
}
Tensor photometric_autocast(PHOTO_ARGS) {
  c10::impl::ExcludeDispatchKeyGuard no_autocast(c10::DispatchKey::Autocast);
  return photometric_op(
      autocast_image(img), autocast_image(target), autocast_weight(weight), l1_weight, ssim_weight, window_size, sigma, data_range, valid);
}

} // namespace

TORCH_LIBRARY_FRAGMENT(drtk_amd_ext, m) {
  m.def("ssim(Tensor img, Tensor target, Tensor? weight, int window_size, float sigma, float data_range, bool valid) -> Tensor");
  m.def("ssim_map(Tensor img, Tensor target, int window_size, float sigma, float data_range, bool valid) -> Tensor");
  m.def(
      "photometric_loss(Tensor img, Tensor target, Tensor? weight, float l1_weight, float ssim_weight, int window_size, float sigma, "
      "float data_range, bool valid) -> Tensor");
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, Autograd, m) {
  m.impl("ssim", &ssim_autograd);
  m.impl("ssim_map", &ssim_map_autograd);
  m.impl("photometric_loss", &photometric_autograd);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, Autocast, m) {
  m.impl("ssim", ssim_autocast);
  m.impl("ssim_map", ssim_map_autocast);
  m.impl("photometric_loss", photometric_autocast);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CUDA, m) {
  m.impl("ssim", &ssim_hip);
  m.impl("ssim_map", &ssim_map_hip);
  m.impl("photometric_loss", &photometric_hip);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CPU, m) {
  m.impl("ssim", &ssim_cpu);
  m.impl("ssim_map", &ssim_map_cpu);
  m.impl("photometric_loss", &photometric_cpu);
}
