"""The definition of `drtk_amd.ssim` / `drtk_amd.photometric_loss` restated with PyTorch's own pieces, in the dtype of its
inputs (float64 for the checks, float32 for the error of the formulation itself) on whatever device they live on: grouped
`conv2d`, row then column.  `gradient()` is the closed form the backward kernel evaluates; tests/test_image_loss_host.py
holds it against autograd of the forward here.  Also the seeded inputs the tests and profiles/image_loss_bench.py share,
and the structural cases (STRUCTURAL_CASES) that the GPU tests, the guarded driver and the host test have in common."""
import torch as th
import torch.nn.functional as F


def window(window_size, sigma, dtype=th.float64, device="cpu"):
    """g[i] = exp(-(i - r)^2 / (2 sigma^2)), normalised to sum 1, computed in double."""
    r = window_size // 2
    i = th.arange(window_size, dtype=th.float64) - r
    g = th.exp(-(i * i) / (2.0 * float(sigma) ** 2))
    return (g / g.sum()).to(dtype).to(device)


def blur(z, g, valid):
    """G*z per channel: zeros outside the image, or (`valid`) only the windows inside it."""
    C, k = z.shape[1], g.numel()
    pad = 0 if valid else k // 2
    z = F.conv2d(z, g.reshape(1, 1, 1, k).repeat(C, 1, 1, 1), groups=C, padding=(0, pad))
    return F.conv2d(z, g.reshape(1, 1, k, 1).repeat(C, 1, 1, 1), groups=C, padding=(pad, 0))


def _terms(x, y, window_size, sigma, data_range, padding):
    assert padding in ("same", "valid")
    valid = padding == "valid"
    g = window(window_size, sigma, x.dtype, x.device)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mu_x, mu_y = blur(x, g, valid), blur(y, g, valid)
    s_x = blur(x * x, g, valid) - mu_x * mu_x
    s_y = blur(y * y, g, valid) - mu_y * mu_y
    s_xy = blur(x * y, g, valid) - mu_x * mu_y
    A1, A2 = 2 * mu_x * mu_y + c1, 2 * s_xy + c2
    B1, B2 = mu_x * mu_x + mu_y * mu_y + c1, s_x + s_y + c2
    return mu_x, mu_y, A1, A2, B1, B2


def ssim_map(x, y, window_size=11, sigma=1.5, data_range=1.0, padding="same"):
    _, _, A1, A2, B1, B2 = _terms(x, y, window_size, sigma, data_range, padding)
    return A1 * A2 / (B1 * B2)


def _weight(weight, like):
    """[N,1,H,W] in the images' dtype; None is all ones."""
    if weight is None:
        return like.new_ones(like.shape[0], 1, *like.shape[2:])
    w = weight if weight.ndim == 4 else weight[:, None]
    return w.to(like.dtype)


def _crop(w, window_size, padding):
    r = window_size // 2
    return w[:, :, r:w.shape[2] - r, r:w.shape[3] - r] if padding == "valid" else w


def _mean(values, w):
    """sum(w values) / (C sum w), and 0 where the weights sum to 0 -- decided on the device."""
    num, den = (w * values).sum(), values.shape[1] * w.sum()
    return th.where(den > 0, num / th.where(den > 0, den, th.ones_like(den)), th.zeros_like(num))


def ssim(x, y, weight=None, window_size=11, sigma=1.5, data_range=1.0, padding="same", reduction="mean"):
    S = ssim_map(x, y, window_size, sigma, data_range, padding)
    if reduction == "none":
        assert weight is None
        return S
    return _mean(S, _crop(_weight(weight, x), window_size, padding))


def l1(x, y, weight=None):
    return _mean((x - y).abs(), _weight(weight, x))


def photometric_loss(x, y, weight=None, l1_weight=0.8, ssim_weight=0.2, window_size=11, sigma=1.5, data_range=1.0, padding="same"):
    return l1_weight * l1(x, y, weight) + ssim_weight * (1 - ssim(x, y, weight, window_size, sigma, data_range, padding))


def gradient(x, y, h, window_size=11, sigma=1.5, data_range=1.0, padding="same"):
    """d/dx of sum(h * ssim_map(x, y)) in closed form, h being the upstream gradient on the map's domain:
    dmu = 2 mu_y (A2 - A1) / (B1 B2) - 2 mu_x S (1 / B1 - 1 / B2), dxx = -S / B2, dxy = 2 A1 / (B1 B2),
    grad_x = G*(h dmu) + 2 x G*(h dxx) + y G*(h dxy), the blurs over the maps zero-extended to the image."""
    mu_x, mu_y, A1, A2, B1, B2 = _terms(x, y, window_size, sigma, data_range, padding)
    S = A1 * A2 / (B1 * B2)
    dmu = 2 * mu_y * (A2 - A1) / (B1 * B2) - 2 * mu_x * S * (1 / B1 - 1 / B2)
    dxx = -S / B2
    dxy = 2 * A1 / (B1 * B2)
    g = window(window_size, sigma, x.dtype, x.device)
    off = window_size // 2 if padding == "valid" else 0

    def back(m):
        return blur(F.pad(h * m, [off, off, off, off]), g, False)

    return back(dmu) + 2 * x * back(dxx) + y * back(dxy)


def mean_upstream(weight, like, window_size, padding):
    """h of `ssim(..., reduction="mean")` for an upstream gradient of 1: w / (C sum w) on the map's domain, 0 for a zero sum."""
    w = _crop(_weight(weight, like), window_size, padding)
    den = like.shape[1] * w.sum()
    return th.where(den > 0, w / th.where(den > 0, den, th.ones_like(den)), th.zeros_like(w))


def photometric_gradient(x, y, weight=None, l1_weight=0.8, ssim_weight=0.2, window_size=11, sigma=1.5, data_range=1.0, padding="same"):
    """d/dx of photometric_loss in closed form: the SSIM part through `gradient`, plus l1_weight w sign(x - y) / (C sum w)."""
    h = -ssim_weight * mean_upstream(weight, x, window_size, padding)
    return gradient(x, y, h, window_size, sigma, data_range, padding) + l1_weight * mean_upstream(weight, x, 1, "same") * th.sign(x - y)


def make_images(shape, seed=0, dtype=th.float64, data_range=1.0, device="cpu"):
    """(img, target): target is a smooth pattern whose top third is constant (its variance vanishes there, B2 -> C2 where img
    is flat too), img is target plus Gaussian noise of 0.1, clamped to [0, 1]; both scaled by data_range."""
    N, C, H, W = shape
    gen = th.Generator().manual_seed(seed)
    yy = th.linspace(0, 1, H, dtype=th.float64).view(1, 1, H, 1)
    xx = th.linspace(0, 1, W, dtype=th.float64).view(1, 1, 1, W)
    n = th.arange(N, dtype=th.float64).view(N, 1, 1, 1)
    c = th.arange(C, dtype=th.float64).view(1, C, 1, 1)
    target = 0.5 + 0.25 * th.sin(6.0 * xx + 0.7 * c + 0.3 * n) * th.cos(5.0 * yy - 0.4 * c) + 0.2 * (xx - 0.5) * (yy - 0.5)
    target = target.clamp(0, 1).contiguous()
    target[:, :, :max(H // 3, 1)] = 0.4
    img = (target + 0.1 * th.randn(shape, generator=gen, dtype=th.float64)).clamp(0, 1)
    return (img * data_range).to(dtype).to(device), (target * data_range).to(dtype).to(device)


def make_distinct_views(shape, seed=0, dtype=th.float64, data_range=1.0, device="cpu", noise=0.03):
    """(img, target) for the cases with many partial sums, where ONE view's share of a mean of up to 513 views must stand
    100 x above the float32 tolerance (tests/test_image_loss_host.py holds them to that).  `make_images` cannot deliver it
    at any noise, for two reasons this removes.  Its views have nearly the same statistics, so leaving one out moves a mean
    of N views by far less than 1 / N.  And where its target is flat B2 falls to C2, where the float32 formulation is off by
    1e-4: that error sets the tolerance, and 400 x 1e-4 is more than any view of 257 can move a mean.
    Here the target is a checkerboard of dark [0, 0.2] and bright [0.8, 1] pixels, each with a value of its own: every
    window, also the narrow one of window_size 3, holds both, so B2 stays near 0.2 and the formulation's error near 1e-6.
    In the even views img is the target plus Gaussian noise, S near 1; in the odd views it is the NEGATIVE of the target plus
    noise, S near -0.6 and |x - y| near 0.8: every view is about 0.8 from the mean of S."""
    N, C, H, W = shape
    gen = th.Generator().manual_seed(seed)
    yy, xx = th.arange(H).view(1, 1, H, 1), th.arange(W).view(1, 1, 1, W)
    bright = ((yy + xx) % 2 == 0).to(th.float64)
    target = 0.2 * th.rand(shape, generator=gen, dtype=th.float64) + 0.8 * bright
    flip = (th.arange(N) % 2 == 1).view(N, 1, 1, 1)
    img = (th.where(flip, 1.0 - target, target) + noise * th.randn(shape, generator=gen, dtype=th.float64)).clamp(0, 1)
    return (img * data_range).to(dtype).to(device), (target * data_range).to(dtype).to(device)


# The structural cases of the GPU tests, of tests/guarded_added_ops.py and of the host test that proves what they reach:
# name -> (shape, window_size, paddings, inputs).  Each is the smallest shape that reaches its path: a tile of the kernels
# is 32 x 32, an interior tile needs three on an axis, the one-workgroup finalize kernel takes 256 slots per pass.
STRUCTURAL_CASES = {
    "interior_tiles": ((1, 2, 97, 99), 11, ("same", "valid"), "images"),  # 4 x 4 tiles; "valid": 87 x 89, 3 x 3, one true interior tile
    "five_by_two": ((2, 1, 40, 131), 3, ("same", "valid"), "images"),     # tiles_x = 5 != tiles_y = 2, two views
    "slots256": ((256, 1, 8, 9), 3, ("same",), "distinct_views"),         # a tile per view: the finalize loop ends after one pass
    "slots257": ((257, 1, 8, 9), 3, ("same",), "distinct_views"),         # thread 0 takes a second slot
    "slots513": ((513, 1, 8, 9), 3, ("same",), "distinct_views"),         # ... and a third: the order within a thread
    "tiles_and_views": ((33, 1, 75, 75), 11, ("same", "valid"), "distinct_views"),  # 3 x 3 tiles x 33 views = 297 slots
}
SLOT_CASES = [name for name, c in STRUCTURAL_CASES.items() if c[3] == "distinct_views"]
MAKERS = {(c[0], c[1]): c[3] for c in STRUCTURAL_CASES.values()}


def case_inputs(shape, k, dtype=th.float64, data_range=1.0, device="cpu"):
    """(img, target) of the case (shape, window_size): `make_distinct_views` for the many-slot cases, `make_images` otherwise."""
    maker = make_distinct_views if MAKERS.get((tuple(shape), k)) == "distinct_views" else make_images
    return maker(tuple(shape), seed=sum(shape) + k, dtype=dtype, data_range=data_range, device=device)


def tile_constants(root):
    """(kIlTileW, kIlTileH, kIlSums, kBlock) as drtk_amd/csrc spells them."""
    import os
    import re

    src = open(os.path.join(root, "drtk_amd", "csrc", "image_loss.hip")).read() + open(os.path.join(root, "drtk_amd", "csrc", "common.hpp")).read()
    return tuple(int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) for name in ("kIlTileW", "kIlTileH", "kIlSums", "kBlock"))


def make_mask(shape, seed=0, device="cpu"):
    """A foreground mask [N,H,W] with holes: a disc per view less a few rectangles, bool."""
    N, _, H, W = shape
    gen = th.Generator().manual_seed(1000 + seed)
    yy = th.arange(H, dtype=th.float64).view(1, H, 1)
    xx = th.arange(W, dtype=th.float64).view(1, 1, W)
    cy = (0.35 + 0.3 * th.rand(N, 1, 1, generator=gen, dtype=th.float64)) * H
    cx = (0.35 + 0.3 * th.rand(N, 1, 1, generator=gen, dtype=th.float64)) * W
    m = ((yy - cy) / (0.45 * H + 1)) ** 2 + ((xx - cx) / (0.45 * W + 1)) ** 2 < 1.0
    holes = th.rand(N, H, W, generator=gen, dtype=th.float64) < 0.15
    m = m & ~holes
    m[:, H // 2:H // 2 + max(H // 8, 1), W // 4:W // 4 + max(W // 6, 1)] = False
    return m.to(device)
