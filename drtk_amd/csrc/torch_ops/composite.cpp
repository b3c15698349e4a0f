// drtk_amd_ext::composite_layers -- front-to-back compositing of K layers, over drtk_amd_composite_layers /
// drtk_amd_composite_layers_backward (include/drtk_amd.h).  No reference counterpart.  Host-only C++; the CPU key raises.
#include "common.hpp"

#include <array>

namespace {
using namespace drtk_amd_torch;
using c10::optional;

bool has(const optional<Tensor>& t) {
  return t.has_value() && t->defined();
}

// color [N,K,C,H,W] with alpha [N,K,H,W] or [N,K,1,H,W];  without alpha, color is rgba [N,K,C+1,H,W], alpha last.
// Returns the alpha to use as [N,K,H,W] and narrows `color` to its C colour channels (views, nothing is copied).
struct Layers {
  Tensor color, alpha;
};
Layers composite_check(
    const Tensor& color_in, const optional<Tensor>& alpha_in, const optional<Tensor>& index_img, const optional<Tensor>& background) {
  TORCH_CHECK(color_in.defined(), "composite_layers(): expected color to be defined");
  TORCH_CHECK(
      color_in.is_floating_point(), "composite_layers(): expected color to have floating point type, but color has ",
      color_in.dtype());
  TORCH_CHECK(color_in.layout() == at::kStrided, "composite_layers(): expected all inputs to have torch.strided layout");
  TORCH_CHECK(
      color_in.dim() == 5, "composite_layers(): expected color.ndim == 5 ([N, K, C, H, W]), but got color with sizes ",
      color_in.sizes());
  Layers l;
  if (has(alpha_in)) {
    const Tensor& alpha = *alpha_in;
    TORCH_CHECK(
        alpha.dim() == 4 || (alpha.dim() == 5 && alpha.size(2) == 1),
        "composite_layers(): expected alpha to be [N, K, H, W] or [N, K, 1, H, W], but got alpha with sizes ", alpha.sizes());
    l.alpha = alpha.dim() == 5 ? alpha.select(2, 0) : alpha;
    l.color = color_in;
    TORCH_CHECK(
        l.alpha.size(0) == l.color.size(0) && l.alpha.size(1) == l.color.size(1) && l.alpha.size(2) == l.color.size(3) &&
            l.alpha.size(3) == l.color.size(4),
        "composite_layers(): expected alpha to match color in N, K, H and W, but got color with sizes ", color_in.sizes(),
        " and alpha with sizes ", alpha.sizes());
    TORCH_CHECK(
        alpha.dtype() == color_in.dtype(), "composite_layers(): expected alpha to have the type of color, but color has ",
        color_in.dtype(), " and alpha has ", alpha.dtype());
    TORCH_CHECK(
        alpha.device() == color_in.device(), "composite_layers(): expected all inputs to be on same device, but color is on ",
        color_in.device(), " and alpha on ", alpha.device());
    TORCH_CHECK(alpha.layout() == at::kStrided, "composite_layers(): expected all inputs to have torch.strided layout");
  } else {
    TORCH_CHECK(
        color_in.size(2) >= 2,
        "composite_layers(): without alpha, color must be rgba [N, K, C + 1, H, W] with alpha as its last channel, but got color "
        "with sizes ",
        color_in.sizes());
    l.color = color_in.narrow(2, 0, color_in.size(2) - 1);
    l.alpha = color_in.select(2, color_in.size(2) - 1);
  }
  const int64_t N = l.color.size(0), K = l.color.size(1), C = l.color.size(2), H = l.color.size(3), W = l.color.size(4);
  TORCH_CHECK(
      K >= 1 && K <= DRTK_AMD_MAX_RASTER_LAYERS, "composite_layers(): the number of layers must be in [1, ",
      DRTK_AMD_MAX_RASTER_LAYERS, "], but got ", K);
  TORCH_CHECK(C >= 1, "composite_layers(): expected at least one colour channel, but got color with sizes ", color_in.sizes());
  TORCH_CHECK(
      H * W < (int64_t(1) << 31), "composite_layers(): expected H * W to be less than 2147483648, but got H: ", H, ", W: ", W);
  if (has(index_img)) {
    const Tensor& idx = *index_img;
    TORCH_CHECK(idx.dtype() == at::kInt, "composite_layers(): expected index_img to have int32 type, but index_img has ", idx.dtype());
    TORCH_CHECK(
        idx.dim() == 4 && idx.size(0) == N && idx.size(1) == K && idx.size(2) == H && idx.size(3) == W,
        "composite_layers(): expected index_img to be [N, K, H, W] = [", N, ", ", K, ", ", H, ", ", W, "], but got index_img with sizes ",
        idx.sizes());
    TORCH_CHECK(
        idx.device() == color_in.device(), "composite_layers(): expected all inputs to be on same device, but color is on ",
        color_in.device(), " and index_img on ", idx.device());
    TORCH_CHECK(idx.layout() == at::kStrided, "composite_layers(): expected all inputs to have torch.strided layout");
  }
  if (has(background)) {
    const Tensor& bg = *background;
    TORCH_CHECK(
        bg.dim() == 4 && bg.size(0) == N && bg.size(1) == C && bg.size(2) == H && bg.size(3) == W,
        "composite_layers(): expected background to be [N, C, H, W] = [", N, ", ", C, ", ", H, ", ", W,
        "], but got background with sizes ", bg.sizes());
    TORCH_CHECK(
        bg.dtype() == color_in.dtype(), "composite_layers(): expected background to have the type of color, but color has ",
        color_in.dtype(), " and background has ", bg.dtype());
    TORCH_CHECK(
        bg.device() == color_in.device(), "composite_layers(): expected all inputs to be on same device, but color is on ",
        color_in.device(), " and background on ", bg.device());
    TORCH_CHECK(bg.layout() == at::kStrided, "composite_layers(): expected all inputs to have torch.strided layout");
  }
  return l;
}

// the last two dimensions form a contiguous H x W plane (planes of at most one element always do)
bool planes_contiguous(const Tensor& t) {
  const int64_t d = t.dim(), H = t.size(d - 2), W = t.size(d - 1);
  return (W <= 1 || t.stride(d - 1) == 1) && (H <= 1 || t.stride(d - 2) == W);
}

// What the C ABI takes of the inputs: tensors whose planes are not contiguous are copied once, everything else is read in place.
struct Prepared {
  Tensor color, alpha, index, bg; // holders
  int64_t cs[3], as[2], bg_sN;
  int64_t N, K, C, H, W;
  const int32_t* index_ptr() const { return index.defined() ? index.data_ptr<int32_t>() : nullptr; }
  const void* bg_ptr() const { return bg.defined() ? bg.data_ptr() : nullptr; }
};
Prepared composite_prepare(const Layers& l, const optional<Tensor>& index_img, const optional<Tensor>& background) {
  Prepared p;
  p.color = planes_contiguous(l.color) ? l.color : l.color.contiguous();
  p.alpha = planes_contiguous(l.alpha) ? l.alpha : l.alpha.contiguous();
  p.N = p.color.size(0), p.K = p.color.size(1), p.C = p.color.size(2), p.H = p.color.size(3), p.W = p.color.size(4);
  for (int i = 0; i < 3; ++i) p.cs[i] = p.color.stride(i);
  for (int i = 0; i < 2; ++i) p.as[i] = p.alpha.stride(i);
  if (has(index_img)) p.index = index_img->contiguous();
  p.bg_sN = 0;
  if (has(background)) {
    const Tensor& bg = *background;
    if (bg.size(0) > 1 && bg.stride(0) == 0) { // one background for all views (expand)
      p.bg = bg.select(0, 0).contiguous();
    } else {
      p.bg = bg.contiguous();
      p.bg_sN = p.C * p.H * p.W;
    }
  }
  return p;
}

std::tuple<Tensor, Tensor> composite_layers_hip(
    const Tensor& color, const optional<Tensor>& alpha, const optional<Tensor>& index_img, const optional<Tensor>& background) {
  const Layers l = composite_check(color, alpha, index_img, background);
  TORCH_CHECK(color.is_cuda(), "composite_layers(): expected all inputs to be on same cuda device");
  const drtk_dtype_t dt = dtype_of(color, "composite_layers");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(color.device());
  const Prepared p = composite_prepare(l, index_img, background);
  auto img = out_empty({p.N, p.C, p.H, p.W}, color.options());
  auto trans = out_empty({p.N, 1, p.H, p.W}, color.options());
  check_status(
      drtk_amd_composite_layers(
          dt, p.color.data_ptr(), p.cs, p.alpha.data_ptr(), p.as, p.index_ptr(), p.bg_ptr(), p.bg_sN, p.N, p.K, p.C, p.H, p.W,
          img.data_ptr(), trans.data_ptr(), current_stream(color)),
      "composite_layers");
  return {img, trans};
}

std::tuple<Tensor, Tensor> composite_layers_cpu(
    const Tensor& color, const optional<Tensor>& alpha, const optional<Tensor>& index_img, const optional<Tensor>& background) {
  composite_check(color, alpha, index_img, background); // a bad call reads the same with and without a device
  no_cpu("composite_layers");
}

std::tuple<Tensor, Tensor> composite_layers_op(
    const Tensor& color, const optional<Tensor>& alpha, const optional<Tensor>& index_img, const optional<Tensor>& background) {
  static auto op = c10::Dispatcher::singleton()
                       .findSchemaOrThrow("drtk_amd_ext::composite_layers", "")
                       .typed<decltype(composite_layers_op)>();
  return op.call(color, alpha, index_img, background);
}

// Gradients of (color, alpha, background); an undefined tensor where none is wanted.  With `rgba` the colour and alpha
// gradients are one [N,K,C+1,H,W] tensor, written through two pointer and stride sets, returned as the first.
std::array<Tensor, 3> composite_layers_backward_hip(
    const Tensor& g_img, const Tensor& g_T, const Tensor& color, const optional<Tensor>& alpha, const optional<Tensor>& index_img,
    const optional<Tensor>& background, bool want_color, bool want_alpha, bool want_bg) {
  const bool rgba = !has(alpha);
  const Layers l = composite_check(color, alpha, index_img, background);
  const drtk_dtype_t dt = dtype_of(color, "composite_layers_backward");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(color.device());
  const Prepared p = composite_prepare(l, index_img, background);
  const auto type = color.scalar_type();
  Tensor gi, gt; // contiguous, in the op's type
  if (g_img.defined()) gi = g_img.to(type).contiguous();
  if (g_T.defined()) gt = g_T.to(type).contiguous();
  std::array<Tensor, 3> grads;
  Tensor gc_view, ga_view;
  if (rgba) {
    if (want_color) { // covers both
      grads[0] = out_empty(color.sizes(), color.options());
      gc_view = grads[0].narrow(2, 0, p.C), ga_view = grads[0].select(2, p.C);
    }
  } else {
    if (want_color) grads[0] = gc_view = out_empty(color.sizes(), color.options());
    if (want_alpha) {
      grads[1] = out_empty(alpha->sizes(), color.options());
      ga_view = alpha->dim() == 5 ? grads[1].select(2, 0) : grads[1];
    }
  }
  if (want_bg) grads[2] = out_empty({p.N, p.C, p.H, p.W}, color.options());
  int64_t gcs[3] = {0, 0, 0}, gas[2] = {0, 0};
  if (gc_view.defined()) {
    for (int i = 0; i < 3; ++i) gcs[i] = gc_view.stride(i);
  }
  if (ga_view.defined()) {
    for (int i = 0; i < 2; ++i) gas[i] = ga_view.stride(i);
  }
  check_status(
      drtk_amd_composite_layers_backward(
          dt, gi.defined() ? gi.data_ptr() : nullptr, gt.defined() ? gt.data_ptr() : nullptr, p.color.data_ptr(), p.cs,
          p.alpha.data_ptr(), p.as, p.index_ptr(), p.bg_ptr(), p.bg_sN, p.N, p.K, p.C, p.H, p.W,
          gc_view.defined() ? gc_view.data_ptr() : nullptr, gcs, ga_view.defined() ? ga_view.data_ptr() : nullptr, gas,
          grads[2].defined() ? grads[2].data_ptr() : nullptr, current_stream(color)),
      "composite_layers_backward");
  return grads;
}

class CompositeLayersFunction : public torch::autograd::Function<CompositeLayersFunction> {
 public:
  static tensor_list forward(
      AutogradContext* ctx, const Tensor& color, const optional<Tensor>& alpha, const optional<Tensor>& index_img,
      const optional<Tensor>& background) {
    ctx->set_materialize_grads(false);
    const bool has_alpha = has(alpha), has_index = has(index_img), has_bg = has(background);
    ctx->saved_data["data"] = std::make_tuple(
        color.requires_grad(), has_alpha && alpha->requires_grad(), has_bg && background->requires_grad(), has_alpha, has_index,
        has_bg);
    std::tuple<Tensor, Tensor> out;
    {
      at::AutoDispatchBelowADInplaceOrView g;
      out = composite_layers_op(color, alpha, index_img, background);
    }
    tensor_list saved = {color};
    if (has_alpha) saved.push_back(*alpha);
    if (has_index) saved.push_back(*index_img);
    if (has_bg) saved.push_back(*background);
    ctx->save_for_backward(saved);
    return {std::get<0>(out), std::get<1>(out)};
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grad_outputs) {
    bool want_color, want_alpha, want_bg, has_alpha, has_index, has_bg;
    std::tie(want_color, want_alpha, want_bg, has_alpha, has_index, has_bg) =
        ctx->saved_data["data"].to<std::tuple<bool, bool, bool, bool, bool, bool>>();
    tensor_list grads(4); // index_img gets none
    if (!(want_color || want_alpha || want_bg) || !(grad_outputs[0].defined() || grad_outputs[1].defined())) return grads;
    // the backward is a kernel, not a graph of differentiable operations: with create_graph=True its result would pass for a constant
    TORCH_CHECK(
        !at::GradMode::is_enabled(),
        "composite_layers(): double backward (create_graph=True) is not supported by drtk_amd's composite_layers kernels");
    const auto saved = ctx->get_saved_variables();
    size_t at = 1;
    optional<Tensor> alpha, index_img, background;
    if (has_alpha) alpha = saved[at++];
    if (has_index) index_img = saved[at++];
    if (has_bg) background = saved[at++];
    const auto g = composite_layers_backward_hip(
        grad_outputs[0], grad_outputs[1], saved[0], alpha, index_img, background, want_color, want_alpha, want_bg);
    if (want_color) grads[0] = g[0];
    if (want_alpha) grads[1] = g[1];
    if (want_bg) grads[3] = g[2];
    return grads;
  }
};

std::tuple<Tensor, Tensor> composite_layers_autograd(
    const Tensor& color, const optional<Tensor>& alpha, const optional<Tensor>& index_img, const optional<Tensor>& background) {
  const auto out = CompositeLayersFunction::apply(color, alpha, index_img, background);
  return {out[0], out[1]};
}

optional<Tensor> to_float(const optional<Tensor>& t) {
  return has(t) ? optional<Tensor>(at::autocast::cached_cast(at::kFloat, *t)) : t;
}

std::tuple<Tensor, Tensor> composite_layers_autocast(
    const Tensor& color, const optional<Tensor>& alpha, const optional<Tensor>& index_img, const optional<Tensor>& background) {
  c10::impl::ExcludeDispatchKeyGuard no_autocast(c10::DispatchKey::Autocast);
  return composite_layers_op(at::autocast::cached_cast(at::kFloat, color), to_float(alpha), index_img, to_float(background));
}

} // namespace

TORCH_LIBRARY_FRAGMENT(drtk_amd_ext, m) {
  m.def("composite_layers(Tensor color, Tensor? alpha, Tensor? index_img, Tensor? background) -> (Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, Autograd, m) {
  m.impl("composite_layers", &composite_layers_autograd);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, Autocast, m) {
  m.impl("composite_layers", composite_layers_autocast);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CUDA, m) {
  m.impl("composite_layers", &composite_layers_hip);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CPU, m) {
  m.impl("composite_layers", &composite_layers_cpu);
}
