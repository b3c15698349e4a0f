// grid_scatter_ext::grid_scatter_2d -- src/grid_scatter/grid_scatter_module.cpp:16-152 and the host side of
// src/grid_scatter/grid_scatter_kernel.cu:624-788.
#include "common.hpp"

namespace {
using namespace drtk_amd_torch;

// grid: read in place where its pixels are evenly spaced in memory (common.hpp: prep_grid), like the reference, which
// reads it through its strides (grid_scatter_kernel.cu:438-451).
Tensor grid_scatter_2d_hip(
    const Tensor& input, const Tensor& grid, int64_t output_height, int64_t output_width, int64_t padding_mode,
    int64_t interpolation_mode, bool align_corners) {
  const char* op = "grid_scatter";
  TORCH_CHECK(input.defined() && grid.defined(), op, "(): input and grid must both be defined tensors");
  TORCH_CHECK(
      output_height > 0 && output_width > 0, op, "(): output_height and output_width must be positive, got ", output_height,
      " and ", output_width);
  TORCH_CHECK(
      input.device() == grid.device() && input.is_cuda(), op, "(): input and grid must live on one HIP device, got ",
      input.device(), " and ", grid.device());
  TORCH_CHECK(
      input.is_floating_point() && grid.is_floating_point() && input.scalar_type() == grid.scalar_type(), op,
      "(): input and grid must share one floating point dtype, got ", input.scalar_type(), " and ", grid.scalar_type());
  TORCH_CHECK(
      input.layout() == at::kStrided && grid.layout() == at::kStrided, op, "(): input and grid must be strided tensors");
  TORCH_CHECK(
      input.dim() == 4 && grid.dim() == 4, op, "(): input must be [N,C,H,W] and grid [N,H,W,2], got ", input.sizes(),
      " and ", grid.sizes());
  TORCH_CHECK(
      input.size(0) == grid.size(0) && input.size(2) == grid.size(1) && input.size(3) == grid.size(2), op,
      "(): grid must have input's batch size, height and width, got input ", input.sizes(), " and grid ", grid.sizes());
  TORCH_CHECK(grid.size(3) == 2, op, "(): the last dimension of grid must have size 2, got grid ", grid.sizes());
  TORCH_CHECK(
      padding_mode >= 0 && padding_mode <= 2 && (interpolation_mode == 0 || interpolation_mode == 2), op,
      "(): unsupported padding_mode / interpolation_mode (bilinear and bicubic only)");
  const drtk_dtype_t dt = dtype_of(input, "grid_scatter_2d_kernel");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(input.device());
  const int64_t N = input.size(0), C = input.size(1), H = input.size(2), W = input.size(3);
  const auto in_c = input.contiguous();
  const GridArg ga = prep_grid(grid);
  auto out = out_empty({N, C, output_height, output_width}, input.options()); // zero-filled by the call (N * H * W == 0 too)
  check_status(
      drtk_amd_grid_scatter_2d(
          dt, in_c.data_ptr(), ga.t.data_ptr(), ga.layout, N, C, H, W, output_height, output_width,
          static_cast<int>(padding_mode), static_cast<int>(interpolation_mode), align_corners, out.data_ptr(), nullptr,
          current_stream(input)),
      op);
  return out;
}

std::tuple<Tensor, Tensor> grid_scatter_2d_backward_hip(
    const Tensor& grad_output, const Tensor& input, const Tensor& grid, int64_t padding_mode, int64_t interpolation_mode,
    bool align_corners, bool grid_requires_grad, bool input_requires_grad) {
  const drtk_dtype_t dt = dtype_of(input, "grid_scatter_2d_backward_kernel");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(input.device());
  const int64_t N = input.size(0), C = input.size(1), H = input.size(2), W = input.size(3);
  const auto in_c = input.contiguous();
  const auto go_c = grad_output.to(input.scalar_type()).contiguous();
  const GridArg ga = prep_grid(grid);
  Tensor grad_input, grad_grid; // what is not asked for stays undefined
  if (input_requires_grad) grad_input = out_empty({N, C, H, W}, input.options());
  // laid out like the grid it belongs to: the gradient of a permuted channel-first uv image arrives channel-first at
  // interpolate's backward (the reference allocates it contiguous, grid_scatter_kernel.cu:747)
  if (grid_requires_grad) grad_grid = at::empty_strided(ga.t.sizes(), ga.t.strides(), grid.options());
  check_status(
      drtk_amd_grid_scatter_2d_backward(
          dt, go_c.data_ptr(), in_c.data_ptr(), ga.t.data_ptr(), ga.layout, N, C, H, W, go_c.size(2), go_c.size(3),
          static_cast<int>(padding_mode), static_cast<int>(interpolation_mode), align_corners,
          input_requires_grad ? grad_input.data_ptr() : nullptr, grid_requires_grad ? grad_grid.data_ptr() : nullptr, ga.layout,
          current_stream(input)),
      "grid_scatter_backward");
  return {grad_input, grad_grid};
}

Tensor grid_scatter_2d_cpu(const Tensor&, const Tensor&, int64_t, int64_t, int64_t, int64_t, bool) {
  no_cpu("grid_scatter");
}

Tensor grid_scatter_2d_op(
    const Tensor& input, const Tensor& grid, int64_t output_height, int64_t output_width, int64_t padding_mode,
    int64_t interpolation_mode, bool align_corners) {
  static auto op = c10::Dispatcher::singleton()
                       .findSchemaOrThrow("grid_scatter_ext::grid_scatter_2d", "")
                       .typed<decltype(grid_scatter_2d_op)>();
  return op.call(input, grid, output_height, output_width, padding_mode, interpolation_mode, align_corners);
}

class GridScatter2DFunction : public torch::autograd::Function<GridScatter2DFunction> {
 public:
  static tensor_list forward(
      AutogradContext* ctx, const Tensor& input, const Tensor& grid, int64_t output_height, int64_t output_width,
      int64_t padding_mode, int64_t interpolation_mode, bool align_corners) {
    ctx->set_materialize_grads(false);
    ctx->save_for_backward({input, grid});
    ctx->saved_data["data"] =
        std::make_tuple(grid.requires_grad(), input.requires_grad(), padding_mode, interpolation_mode, align_corners);
    at::AutoDispatchBelowADInplaceOrView g;
    return {grid_scatter_2d_op(input, grid, output_height, output_width, padding_mode, interpolation_mode, align_corners)};
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grad_outputs) {
    bool grid_requires_grad, input_requires_grad, align_corners;
    int64_t padding_mode, interpolation_mode;
    std::tie(grid_requires_grad, input_requires_grad, padding_mode, interpolation_mode, align_corners) =
        ctx->saved_data["data"].to<std::tuple<bool, bool, int64_t, int64_t, bool>>();
    tensor_list grads(7);
    if ((!grid_requires_grad && !input_requires_grad) || !grad_outputs[0].defined()) return grads; // nothing is computed
    const auto saved = ctx->get_saved_variables();
    auto g = grid_scatter_2d_backward_hip(
        grad_outputs[0], saved[0], saved[1], padding_mode, interpolation_mode, align_corners, grid_requires_grad,
        input_requires_grad);
    grads[0] = std::get<0>(g);
    grads[1] = std::get<1>(g);
    return grads;
  }
};

Tensor grid_scatter_2d_autograd(
    const Tensor& input, const Tensor& grid, int64_t output_height, int64_t output_width, int64_t padding_mode,
    int64_t interpolation_mode, bool align_corners) {
  return GridScatter2DFunction::apply(
      input, grid, output_height, output_width, padding_mode, interpolation_mode, align_corners)[0];
}

Tensor grid_scatter_2d_autocast(
    const Tensor& input, const Tensor& grid, int64_t output_height, int64_t output_width, int64_t padding_mode,
    int64_t interpolation_mode, bool align_corners) {
  c10::impl::ExcludeDispatchKeyGuard no_autocast(c10::DispatchKey::Autocast);
  return grid_scatter_2d_op(
      at::autocast::cached_cast(at::kFloat, input), at::autocast::cached_cast(at::kFloat, grid), output_height,
      output_width, padding_mode, interpolation_mode, align_corners);
}

} // namespace

// schema: verbatim from the reference
TORCH_LIBRARY(grid_scatter_ext, m) {
  m.def(
      "grid_scatter_2d(Tensor input, Tensor grid, int output_height, int output_width, int padding_mode, int interpolation_mode, bool align_corners) -> Tensor");
}
TORCH_LIBRARY_IMPL(grid_scatter_ext, Autograd, m) {
  m.impl("grid_scatter_2d", &grid_scatter_2d_autograd);
}
TORCH_LIBRARY_IMPL(grid_scatter_ext, Autocast, m) {
  m.impl("grid_scatter_2d", grid_scatter_2d_autocast);
}
TORCH_LIBRARY_IMPL(grid_scatter_ext, CUDA, m) {
  m.impl("grid_scatter_2d", &grid_scatter_2d_hip);
}
TORCH_LIBRARY_IMPL(grid_scatter_ext, CPU, m) { // the reference registers no CPU kernel either
  m.impl("grid_scatter_2d", &grid_scatter_2d_cpu);
}
