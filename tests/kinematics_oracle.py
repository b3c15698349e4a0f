"""TEST INFRASTRUCTURE -- an oracle for drtk_amd.forward_kinematics that shares nothing with the package: the local rotation
is torch.linalg.matrix_exp of the skew matrix (exact and smooth at r = 0, no closed form, no threshold), every joint is a
homogeneous 4x4 matrix, the tree is a Python loop over the joints (G_j = G_p @ [[R_j, c_j - c_p], [0, 1]]), the skinning
matrix is G_j @ [[I, -c_j], [0, 1]], and every gradient is autograd's of (transforms * gA).sum() + (posed * gP).sum().  It
runs in the dtype it is given.

A case is a dict: "rot_leaf" and "rot_view" (the leaf the gradient is taken to, and the function that makes `rotations`
from it -- a slice of a larger parameter tensor stays a slice), "joints_leaf" / "joints_view" likewise, "parents" (a list),
"translation" (or None), "gA" / "gP" (the output gradients; None: that output is not used).  CASES are the smallest trees at
which the kernels of csrc/kinematics.hip can go wrong (the cap and the Taylor thresholds are read from the source);
build_case(seed) draws random trees for the fuzz rows."""
import math
import os
import re

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(name):
    src = open(os.path.join(ROOT, "drtk_amd", "csrc", "kinematics.hip")).read()
    m = re.search(r"constexpr\s+(?:int|double)\s+" + name + r"\s*=\s*([0-9.eE+-]+)\s*;", src)
    assert m, f"csrc/kinematics.hip no longer defines {name}"
    return float(m.group(1))


MAX_JOINTS = int(_constant("kFkMaxJoints"))
THETA0 = {th.float32: math.sqrt(_constant("kFkTaylorTheta2F32")), th.float64: math.sqrt(_constant("kFkTaylorTheta2F64"))}

BODY24 = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]  # SMPL
HAND16 = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14]  # MANO


def _skew(r):
    x, y, z = r.unbind(-1)
    o = th.zeros_like(x)
    return th.stack([th.stack([o, -z, y], -1), th.stack([z, o, -x], -1), th.stack([-y, x, o], -1)], -2)


def _hom(rot, t):
    """[..., 3, 3], [..., 3] -> [..., 4, 4]"""
    top = th.cat([rot, t[..., None]], -1)
    bottom = th.zeros_like(top[..., :1, :])
    bottom[..., 0, 3] = 1
    return th.cat([top, bottom], -2)


def forward_kinematics(rotations, joints, parents, translation=None):
    """-> (transforms [N,J,3,4], posed_joints [N,J,3])"""
    n, num_j = rotations.shape[0], rotations.shape[1]
    rot = rotations if rotations.dim() == 4 else th.linalg.matrix_exp(_skew(rotations))
    c = (joints if joints.dim() == 3 else joints[None]).expand(n, -1, -1)
    eye = th.eye(3, dtype=rot.dtype, device=rot.device).expand(n, 3, 3)
    world, skinning = [], []
    for j, p in enumerate([int(x) for x in parents]):
        if p < 0:
            g = _hom(rot[:, j], c[:, j] if translation is None else c[:, j] + translation)
        else:
            g = world[p] @ _hom(rot[:, j], c[:, j] - c[:, p])
        world.append(g)
        skinning.append(g @ _hom(eye, -c[:, j]))
    world, skinning = th.stack(world, 1), th.stack(skinning, 1)
    assert world.shape == (n, num_j, 4, 4)
    return skinning[:, :, :3, :], world[:, :, :3, 3]


KEYS = ("transforms", "posed", "grad_rot", "grad_joints", "grad_tr")


def results(fn, case, dtype, device="cpu", parents=None):
    """{"transforms", "posed", "grad_rot", "grad_joints", "grad_tr"} of `fn` (this oracle, or the package) on copies of the
    case's inputs in `dtype` on `device`; the gradients have the shapes of the leaves (grad_tr: [N,3], zeros without a
    translation).  `parents` replaces the case's list (a tensor, another dtype)."""
    rl = case["rot_leaf"].to(dtype).to(device).clone().requires_grad_(True)
    jl = case["joints_leaf"].to(dtype).to(device).clone().requires_grad_(True)
    rot, joints = case["rot_view"](rl), case["joints_view"](jl)
    tr = None if case["translation"] is None else case["translation"].to(dtype).to(device).clone().requires_grad_(True)
    transforms, posed = fn(rot, joints, case["parents"] if parents is None else parents, tr)
    loss = 0
    if case["gA"] is not None:
        loss = loss + (transforms * case["gA"].to(dtype).to(device)).sum()
    if case["gP"] is not None:
        loss = loss + (posed * case["gP"].to(dtype).to(device)).sum()
    leaves = [rl, jl] + ([tr] if tr is not None else [])
    grads = th.autograd.grad(loss, leaves, allow_unused=True)
    zero = lambda g, like: th.zeros_like(like) if g is None else g  # noqa: E731
    n = rot.shape[0]
    return {"transforms": transforms.detach().cpu(), "posed": posed.detach().cpu(), "grad_rot": zero(grads[0], rl).cpu(),
            "grad_joints": zero(grads[1], jl).cpu(),
            "grad_tr": zero(grads[2], tr).cpu() if tr is not None else th.zeros(n, 3, dtype=dtype)}


def _r(gen, *shape):
    """float64 values that are exact in float32 (one set of inputs for either precision)"""
    return th.randn(*shape, dtype=th.float64, generator=gen).float().double()


def _identity(x):
    return x


def _make(gen, n, parents, pose=None, matrices=False, joints="shared", translation=True, grads="both", rot_layout="plain"):
    num_j = len(parents)
    if matrices:
        rot_leaf = _r(gen, n, num_j, 3, 3) * 0.6 + th.eye(3, dtype=th.float64)
    else:
        rot_leaf = (0.5 * _r(gen, n, num_j, 3) if pose is None else pose).float().double()
    rot_view = _identity
    if rot_layout == "sliced":  # theta[:, 3:].view(N, J, 3): a slice of a larger parameter tensor
        assert not matrices
        rot_leaf = th.cat([_r(gen, n, 3), rot_leaf.reshape(n, -1)], 1)
        rot_view = lambda t: t[:, 3:].view(t.shape[0], -1, 3)  # noqa: E731
    elif rot_layout == "strided":  # every second element of the last dimension(s)
        big = _r(gen, *rot_leaf.shape[:-1], 2 * rot_leaf.shape[-1])
        big[..., ::2] = rot_leaf
        rot_leaf = big
        rot_view = lambda t: t[..., ::2]  # noqa: E731
    c = 0.3 * _r(gen, n if joints == "per_view" else 1, num_j, 3)
    joints_view = _identity
    if joints == "shared":
        c = c[0]
    elif joints == "expanded":
        joints_view = lambda t: t.expand(n, -1, -1)  # noqa: E731
    return {"rot_leaf": rot_leaf, "rot_view": rot_view, "joints_leaf": c.float().double(), "joints_view": joints_view,
            "parents": list(parents), "translation": _r(gen, n, 3) if translation else None,
            "gA": _r(gen, n, num_j, 3, 4) if grads in ("both", "transforms") else None,
            "gP": _r(gen, n, num_j, 3) if grads in ("both", "posed") else None}


def _random_tree(gen, num_j, roots):
    ri = lambda lo, hi: int(th.randint(lo, hi + 1, (1,), generator=gen))  # noqa: E731
    root_at = set([0] + [ri(1, num_j - 1) for _ in range(roots - 1)] if num_j > 1 else [0])
    return [-1 if j in root_at else ri(0, j - 1) for j in range(num_j)]


def _directions(gen, *shape):
    d = th.randn(*shape, 3, dtype=th.float64, generator=gen)
    return d / d.norm(dim=-1, keepdim=True)


def _case(name):
    gen = th.Generator().manual_seed(sum(map(ord, name)))
    chain = lambda k: [-1] + list(range(k - 1))  # noqa: E731
    if name == "root_only":
        return _make(gen, 3, [-1])
    if name == "chain5":
        return _make(gen, 3, chain(5))
    if name == "chain32":
        return _make(gen, 3, chain(32))
    if name == "star70":
        return _make(gen, 3, [-1] + [0] * 69)
    if name == "wide130":
        return _make(gen, 3, [-1, -1] + [0] * 64 + [1] * 64)
    if name == "body24":
        return _make(gen, 3, BODY24)
    if name == "hand16":
        return _make(gen, 3, HAND16)
    if name == "zero_pose":
        return _make(gen, 3, BODY24, pose=th.zeros(3, 24, 3, dtype=th.float64))
    if name == "tiny_pose":
        # |r| at 0.5 x and 2 x either dtype's threshold angle: both sides of the Taylor switch, in both precisions
        angles = th.tensor([0.5 * THETA0[th.float32], 2 * THETA0[th.float32], 0.5 * THETA0[th.float64], 2 * THETA0[th.float64]], dtype=th.float64)
        pose = _directions(gen, 3, 16) * angles.repeat(4)[None, :, None]
        return _make(gen, 3, HAND16, pose=pose)
    if name == "big_angle":
        pose = _directions(gen, 3, 24) * (2.5 * math.pi * th.rand(3, 24, 1, dtype=th.float64, generator=gen))
        pose[0, 0] *= 2.5 * math.pi / pose[0, 0].norm()
        return _make(gen, 3, BODY24, pose=pose)
    if name == "matrices":
        return _make(gen, 3, BODY24, matrices=True)
    if name == "per_view_joints":
        return _make(gen, 3, HAND16, joints="per_view")
    if name == "expanded_joints":
        return _make(gen, 3, HAND16, joints="expanded")
    if name == "one_view":
        return _make(gen, 1, HAND16)
    if name == "no_translation":
        return _make(gen, 3, [-1, 0, -1, 2, 1, 3, 0], translation=False)
    if name == "only_posed_grad":
        return _make(gen, 3, HAND16, grads="posed")
    if name == "only_transforms_grad":
        return _make(gen, 3, HAND16, grads="transforms")
    if name == "sliced_pose":
        return _make(gen, 3, HAND16, rot_layout="sliced")
    if name == "strided_pose":
        return _make(gen, 3, HAND16, rot_layout="strided")
    if name == "strided_matrices":
        return _make(gen, 2, chain(5), matrices=True, rot_layout="strided")
    if name == "at_cap":
        return _make(gen, 2, _random_tree(gen, MAX_JOINTS, 2))
    if name == "past_cap":
        return _make(gen, 2, _random_tree(gen, MAX_JOINTS + 1, 2))
    raise KeyError(name)


CASES = ("root_only", "chain5", "chain32", "star70", "wide130", "body24", "hand16", "zero_pose", "tiny_pose", "big_angle",
         "matrices", "per_view_joints", "expanded_joints", "one_view", "no_translation", "only_posed_grad",
         "only_transforms_grad", "sliced_pose", "strided_pose", "strided_matrices", "at_cap", "past_cap")
SEEDS = tuple(range(30))
_cache = {}


def case(name):
    """The case called `name`, float64 on the CPU; built once, never modified"""
    if name not in _cache:
        _cache[name] = _case(name)
    return _cache[name]


def build_case(seed):
    """A seeded random tree: J in 1 ... 96, 1 to 3 roots, N in 1 ... 5; every layout, argument presence and rotation format"""
    gen = th.Generator().manual_seed(2000 + seed)
    ri = lambda lo, hi: int(th.randint(lo, hi + 1, (1,), generator=gen))  # noqa: E731
    n, num_j = ri(1, 5), ri(1, 96)
    matrices = ri(0, 2) == 0
    layout = ("plain", "strided", "plain" if matrices else "sliced")[ri(0, 2)]
    return _make(gen, n, _random_tree(gen, num_j, min(ri(1, 3), num_j)), matrices=matrices,
                 joints=("shared", "shared3", "per_view", "expanded")[ri(0, 3)], translation=ri(0, 1) == 1,
                 grads=("both", "both", "transforms", "posed")[ri(0, 3)], rot_layout=layout)


def key_case(key):
    return case(key) if isinstance(key, str) else build_case(key)


_ref = {}


def reference(key, dtype):
    """The oracle's results for case(key) (a name) or build_case(key) (a seed) in `dtype`; computed once per pair"""
    if (key, dtype) not in _ref:
        _ref[(key, dtype)] = results(forward_kinematics, key_case(key), dtype)
    return _ref[(key, dtype)]


def leaf_joints(parents):
    """mask [J] of the joints without children"""
    leaf = th.ones(len(parents), dtype=th.bool)
    for p in parents:
        if p >= 0:
            leaf[p] = False
    return leaf
