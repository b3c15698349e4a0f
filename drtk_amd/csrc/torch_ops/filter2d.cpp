// filter2d_ext::{resample_filter, low_pass_filter, downsample, upsample, make_resampling_kernel} -- src/filter2d/module.cpp,
// filter2d.cpp (host side) and filter_weights.cpp.  One kernel entry (drtk_amd_filter2d) behind all four image operators.
#include "common.hpp"

#include <cmath>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

namespace {
using namespace drtk_amd_torch;

// ---- filter design (host, double) -----------------------------------------------------------------------------------
double sinc(double t) { // sin(pi t) / (pi t)
  if (t == 0.0) return 1.0;
  const double a = M_PI * t;
  return std::sin(a) / a;
}

std::vector<float> design_filter(int64_t n_taps, int64_t m, double freq_div, double gain, double alias_guard_band, int64_t filter_type) {
  // distance between pixels 1: sampling rate 1, band limit 1/2; transition half-width (sqrt(2) - 1) * band limit (StyleGAN3)
  const double fh = (std::sqrt(2.0) - 1.0) / 2.0 / freq_div;
  const double fc = 1.0 / 2.0 / freq_div - fh * alias_guard_band;
  const int64_t n = n_taps * m;
  std::vector<double> v(n);
  if (filter_type == 0) { // Kaiser
    const double L = double(n - 1) / double(m);
    const double df = 2.0 * fh / (double(m) / 2.0);
    const double A = 2.285 * double(n - 1) * M_PI * df + 7.95;
    const double beta = A > 50.0 ? 0.1102 * (A - 8.7) : (A < 21.0 ? 0.0 : 0.5842 * std::pow(A - 21.0, 0.4) + 0.07886 * (A - 21.0));
    const double i0_beta = std::cyl_bessel_i(0.0, beta);
    for (int64_t i = 0; i < n; ++i) {
      const double x = (double(i) - double(n - 1) / 2.0) / double(m);
      const double r = L > 0.0 ? 2.0 * x / L : 0.0;
      const double inside = 1.0 - r * r; // 0 at the two ends, up to rounding
      const double w = std::cyl_bessel_i(0.0, beta * std::sqrt(inside > 0.0 ? inside : 0.0)) / i0_beta;
      v[i] = w * 2.0 * fc * sinc(2.0 * fc * x);
    }
  } else { // Lanczos; `a` makes all n taps fall inside the window
    const double a = std::ceil(2.0 * fc * double(n - 1) / 2.0 / double(m));
    for (int64_t i = 0; i < n; ++i) {
      const double x = (double(i) - double(n - 1) / 2.0) / double(m);
      const double t = 2.0 * fc * x;
      v[i] = std::fabs(t) < a ? 2.0 * fc * sinc(t) * sinc(t / a) : 0.0;
    }
  }
  double sum = 0.0;
  for (double e : v) sum += e;
  std::vector<float> out(n);
  for (int64_t i = 0; i < n; ++i) out[i] = static_cast<float>(v[i] / sum * gain);
  return out;
}

// One tensor per (parameters, device), made once: the first call for a key copies host to device (so it belongs before a
// graph capture), every later one returns the cached tensor.
Tensor make_resampling_kernel(
    int64_t n, int64_t m, double freq_div, double gain, double alias_guard_band, int64_t filter_type, c10::Device device) {
  TORCH_CHECK(n >= 1, "make_resampling_kernel(): n must be at least 1, but got ", n);
  TORCH_CHECK(m >= 1, "make_resampling_kernel(): m must be at least 1, but got ", m);
  TORCH_CHECK(n <= (int64_t(1) << 20) / m, "make_resampling_kernel(): n * m must be at most 2^20, but got n ", n, " and m ", m);
  TORCH_CHECK(
      std::isfinite(freq_div) && freq_div > 0.0, "make_resampling_kernel(): freq_div must be finite and greater than 0, but got ",
      freq_div);
  TORCH_CHECK(std::isfinite(gain), "make_resampling_kernel(): gain must be finite, but got ", gain);
  TORCH_CHECK(
      std::isfinite(alias_guard_band) && alias_guard_band >= 0.0,
      "make_resampling_kernel(): alias_guard_band must be finite and non-negative, but got ", alias_guard_band);
  TORCH_CHECK(
      filter_type == 0 || filter_type == 1, "make_resampling_kernel(): filter_type must be Kaiser (0) or Lanczos (1), but got ",
      filter_type);
  using Key = std::tuple<int64_t, int64_t, double, double, double, int64_t, int, int>;
  static std::mutex mu;
  static std::map<Key, Tensor> cache;
  if (device.is_cuda() && !device.has_index()) device = c10::Device(device.type(), c10::hip::current_device());
  const Key key{n, m, freq_div, gain, alias_guard_band, filter_type, static_cast<int>(device.type()), static_cast<int>(device.index())};
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  const std::vector<float> w = design_filter(n, m, freq_div, gain, alias_guard_band, filter_type);
  Tensor t = at::empty({static_cast<int64_t>(w.size())}, at::TensorOptions().dtype(at::kFloat));
  std::copy(w.begin(), w.end(), t.data_ptr<float>());
  if (!device.is_cpu()) t = t.to(device);
  cache.emplace(key, t);
  return t;
}

// ---- the image operators --------------------------------------------------------------------------------------------
drtk_dtype_t filter_dtype_of(const Tensor& x) { // (common.hpp's dtype_of admits float and double only)
  switch (x.scalar_type()) {
    case at::kHalf:
      return DRTK_F16;
    case at::kFloat:
      return DRTK_F32;
    default:
      return DRTK_F64;
  }
}

int64_t floor_half(int64_t a) { // floor(a / 2)
  return a >= 0 ? a / 2 : -((1 - a) / 2);
}
int64_t pad0(int64_t k, int64_t up, int64_t down) {
  if (up == 1 && down == 1) return k / 2;
  return down != 1 ? floor_half(k - down + 1) : floor_half(k + up - 1);
}
int64_t pad1(int64_t k, int64_t up, int64_t down) {
  if (up == 1 && down == 1) return (k - 1) / 2;
  return down != 1 ? floor_half(k - down) : floor_half(k - up);
}

// The checks of the operator, CPU and device tensors alike; returns the output's height and width.
std::pair<int64_t, int64_t> filter_check(const Tensor& x, const Tensor& f, int64_t up, int64_t down, bool reflect, bool backward) {
  TORCH_CHECK(x.defined() && f.defined(), "filter2d: expected x and f not to be undefined");
  TORCH_CHECK(f.device() == x.device(), "filter2d: f must reside on the same device as x, but x is on ", x.device(), " and f on ", f.device());
  TORCH_CHECK(f.scalar_type() == at::kFloat, "filter2d: f must be float32, but got ", f.scalar_type());
  TORCH_CHECK(x.dim() == 4, "filter2d: x must be rank 4 (N, C, H, W), but got size ", x.sizes());
  TORCH_CHECK(f.dim() == 1, "filter2d: f must be rank 1, but got size ", f.sizes());
  TORCH_CHECK(
      x.scalar_type() == at::kHalf || x.scalar_type() == at::kFloat || x.scalar_type() == at::kDouble,
      "filter2d: x dtype must be float16, float32, or float64, but got ", x.scalar_type());
  TORCH_CHECK(x.numel() > 0, "filter2d: x dimensions must be non-empty, but got size ", x.sizes());
  TORCH_CHECK(f.size(0) >= 1, "filter2d: f must have at least one tap");
  TORCH_CHECK(up >= 1, "filter2d: upsampling factor (up) must be at least 1, but got ", up);
  TORCH_CHECK(down >= 1, "filter2d: downsampling factor (down) must be at least 1, but got ", down);
  TORCH_CHECK(up <= 65536 && down <= 65536 && f.size(0) <= (1 << 20), "filter2d: up, down at most 65536 and f at most 2^20 taps");
  const int64_t k = f.size(0), H = x.size(2), W = x.size(3);
  const int64_t total = pad0(k, up, down) + pad1(k, up, down);
  const int64_t lead = backward ? k - 1 - pad0(k, down, up) : pad0(k, up, down);
  TORCH_CHECK(
      lead >= 0 && total - lead >= 0, "filter2d: filter too short for the sampling factors: f has ", k, " taps with up ", up, " and down ", down);
  const int64_t OH = (H * up + total - k + down) / down, OW = (W * up + total - k + down) / down;
  TORCH_CHECK(
      H * up + total - k + down >= down && W * up + total - k + down >= down,
      "filter2d: output must be at least 1x1, but x of size ", x.sizes(), " with ", k, " taps, up ", up, " and down ", down, " gives ",
      OH, "x", OW);
  if (reflect) {
    const int64_t before = (lead + up - 1) / up, after = (total - lead + up - 1) / up;
    TORCH_CHECK(
        before < H && after < H && before < W && after < W, "filter2d: reflection padding of (", before, ", ", after,
        ") must be smaller than the spatial size of x, but x has size ", x.sizes());
  }
  return {OH, OW};
}

Tensor filter_run(const Tensor& x, const Tensor& f, int64_t up, int64_t down, bool reflect, bool backward) {
  const auto out_size = filter_check(x, f, up, down, reflect, backward);
  if (!x.is_cuda()) no_cpu("filter2d");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  const auto x_c = x.contiguous(), f_c = f.contiguous();
  auto y = out_empty({x.size(0), x.size(1), out_size.first, out_size.second}, x.options());
  const int status = drtk_amd_filter2d(
      filter_dtype_of(x), x_c.data_ptr(), f_c.data_ptr<float>(), x.size(0) * x.size(1), x.size(2), x.size(3), f.size(0), up, down,
      reflect ? 1 : 0, backward ? 1 : 0, 0, y.data_ptr(), current_stream(x));
  TORCH_CHECK(
      status != DRTK_ERR_UNSUPPORTED, "filter2d: f with ", f.size(0), " taps, up ", up, " and down ", down,
      " needs more than the 160 KiB of LDS of a compute unit for a single row of outputs: not supported");
  check_status(status, "filter2d");
  return y;
}

// One Function for all four operators.  The backward is the operator again with the factors exchanged and the flag
// flipped, called through this Function: double backward works.
class ResampleFunction : public torch::autograd::Function<ResampleFunction> {
 public:
  static tensor_list forward(
      AutogradContext* ctx, const Tensor& x, const Tensor& f, int64_t up, int64_t down, bool reflect, bool backward) {
    ctx->set_materialize_grads(false);
    Tensor y = filter_run(x, f, up, down, reflect, backward); // (judges the arguments: x is [N,C,H,W] below)
    ctx->save_for_backward({f});
    ctx->saved_data["data"] =
        std::make_tuple(x.requires_grad(), up, down, reflect, backward, x.size(2), x.size(3), static_cast<int64_t>(x.scalar_type()));
    return {y};
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grad_outputs) {
    bool requires_grad, reflect, backward;
    int64_t up, down, H, W, x_type;
    std::tie(requires_grad, up, down, reflect, backward, H, W, x_type) =
        ctx->saved_data["data"].to<std::tuple<bool, int64_t, int64_t, bool, bool, int64_t, int64_t, int64_t>>();
    tensor_list grads(6); // f gets no gradient; the other arguments are not tensors
    if (!requires_grad || !grad_outputs[0].defined()) return grads;
    const auto f = ctx->get_saved_variables()[0];
    const auto& g = grad_outputs[0];
    // the gradient has x's shape only where the decimation divides the image: the reference dies inside autograd otherwise
    const int64_t k = f.size(0);
    const int64_t total = pad0(k, down, up) + pad1(k, down, up);
    const int64_t gh = (g.size(2) * down + total - k + up) / up, gw = (g.size(3) * down + total - k + up) / up;
    TORCH_CHECK(
        gh == H && gw == W, "filter2d backward: the gradient of an input of ", H, "x", W, " comes out ", gh, "x", gw,
        " (up ", up, ", down ", down, ", ", k, " taps): with down > 1 the backward needs H and W to be multiples of down");
    grads[0] = ResampleFunction::apply(g.contiguous().to(static_cast<at::ScalarType>(x_type)), f, down, up, reflect, !backward)[0];
    return grads;
  }
};

Tensor resample_autograd_flag(const Tensor& x, const Tensor& f, int64_t up, int64_t down, bool reflect) {
  return ResampleFunction::apply(x, f, up, down, reflect, false)[0];
}

Tensor filter_for(const Tensor& x, int64_t n, int64_t m, double freq_div, double gain, double alias_guard_band, int64_t filter_type) {
  TORCH_CHECK(x.defined(), "filter2d: expected x not to be undefined");
  return make_resampling_kernel(n, m, freq_div, gain, alias_guard_band, filter_type, x.device());
}

// Autograd key
Tensor resample_filter_autograd(const Tensor& x, const Tensor& f, int64_t up, int64_t down, bool reflect) {
  return resample_autograd_flag(x, f, up, down, reflect);
}
Tensor low_pass_filter_autograd(const Tensor& x, int64_t n, double freq_div, double alias_guard_band, int64_t filter_type, bool reflect) {
  return resample_autograd_flag(x, filter_for(x, n, 1, freq_div, 1.0, alias_guard_band, filter_type), 1, 1, reflect);
}
Tensor downsample_autograd(const Tensor& x, int64_t n, int64_t m, double alias_guard_band, int64_t filter_type, bool reflect) {
  TORCH_CHECK(m >= 1, "filter2d: downsampling factor must be at least 1, but got ", m);
  return resample_autograd_flag(x, filter_for(x, n, m, 1.0, 1.0, alias_guard_band, filter_type), 1, m, reflect);
}
Tensor upsample_autograd(const Tensor& x, int64_t n, int64_t m, double alias_guard_band, int64_t filter_type, bool reflect) {
  TORCH_CHECK(m >= 1, "filter2d: upsampling factor must be at least 1, but got ", m);
  return resample_autograd_flag(x, filter_for(x, n, m, 1.0, double(m), alias_guard_band, filter_type), m, 1, reflect);
}

// CUDA key (and CPU: filter_run judges the arguments first, then fails loudly on a CPU image)
Tensor resample_filter_hip(const Tensor& x, const Tensor& f, int64_t up, int64_t down, bool reflect) {
  return filter_run(x, f, up, down, reflect, false);
}
Tensor low_pass_filter_hip(const Tensor& x, int64_t n, double freq_div, double alias_guard_band, int64_t filter_type, bool reflect) {
  return filter_run(x, filter_for(x, n, 1, freq_div, 1.0, alias_guard_band, filter_type), 1, 1, reflect, false);
}
Tensor downsample_hip(const Tensor& x, int64_t n, int64_t m, double alias_guard_band, int64_t filter_type, bool reflect) {
  TORCH_CHECK(m >= 1, "filter2d: downsampling factor must be at least 1, but got ", m);
  return filter_run(x, filter_for(x, n, m, 1.0, 1.0, alias_guard_band, filter_type), 1, m, reflect, false);
}
Tensor upsample_hip(const Tensor& x, int64_t n, int64_t m, double alias_guard_band, int64_t filter_type, bool reflect) {
  TORCH_CHECK(m >= 1, "filter2d: upsampling factor must be at least 1, but got ", m);
  return filter_run(x, filter_for(x, n, m, 1.0, double(m), alias_guard_band, filter_type), m, 1, reflect, false);
}

} // namespace

// schemas: verbatim from the reference
TORCH_LIBRARY(filter2d_ext, m) {
  m.def("resample_filter(Tensor x, Tensor f, int up, int down, bool reflect) -> Tensor");
  m.def("low_pass_filter(Tensor x, int n, float freq_div, float alias_guard_band, int filter_type, bool reflect) -> Tensor");
  m.def("downsample(Tensor x, int n, int m, float alias_guard_band, int filter_type, bool reflect) -> Tensor");
  m.def("upsample(Tensor x, int n, int m, float alias_guard_band, int filter_type, bool reflect) -> Tensor");
  m.def(
      "make_resampling_kernel(int n, int m, float freq_div, float gain, float alias_guard_band, int filter_type, Device d) -> Tensor",
      &make_resampling_kernel);
}
TORCH_LIBRARY_IMPL(filter2d_ext, Autograd, m) {
  m.impl("resample_filter", &resample_filter_autograd);
  m.impl("low_pass_filter", &low_pass_filter_autograd);
  m.impl("downsample", &downsample_autograd);
  m.impl("upsample", &upsample_autograd);
}
TORCH_LIBRARY_IMPL(filter2d_ext, CUDA, m) {
  m.impl("resample_filter", &resample_filter_hip);
  m.impl("low_pass_filter", &low_pass_filter_hip);
  m.impl("downsample", &downsample_hip);
  m.impl("upsample", &upsample_hip);
}
TORCH_LIBRARY_IMPL(filter2d_ext, CPU, m) { // the package has no CPU path
  m.impl("resample_filter", &resample_filter_hip);
  m.impl("low_pass_filter", &low_pass_filter_hip);
  m.impl("downsample", &downsample_hip);
  m.impl("upsample", &upsample_hip);
}
