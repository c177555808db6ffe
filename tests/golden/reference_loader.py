"""What the tests/golden/make_*.py generators share: finding the reference checkout, getting its Python files into
sys.modules next to stand-ins for what they cannot import here, the patches that let its CUDA-only code run on CPU tensors,
and a few small helpers.  Nothing of the reference is held here; its files are named and loaded from where they lie.

A new generator imports this module at the top and does everything else from main():

    root = reference_root()                     # argv[1], else PDA_REFERENCE, else PDA_REFERENCE_ROOT, else the usage text
    cpu_torch()                                 # the reference's CUDA allocations and .cuda() calls work on CPU tensors
    head, = load(root, "pcdet_ref", MODEL_UTILS + ["models.dense_heads.some_head"], stubs=extension_stubs())

`load` registers the missing parent packages (empty ones, so that no __init__.py of the reference runs), then the stubs,
then executes the named files in order.  A stand-in whose arithmetic is particular to one fixture stays in its generator and
is passed through `stubs`; a patch of one loaded module (`mod.torch = ...`) is applied by the generator to what `load`
returns.  Importing a generator must stay free of side effects: no reading of argv or the environment, nothing loaded or
patched before main() runs (tests/test_golden_loader.py checks that).
"""
import contextlib
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import oracle  # noqa: E402
import roi_pool_restatement  # noqa: E402
import stack_sa_restatement  # noqa: E402

# the files most model generators need before their own, in an order in which each finds what it imports
MODEL_UTILS = ["utils.common_utils", "utils.box_utils", "utils.loss_utils", "utils.box_coder_utils",
               "ops.iou3d_nms.iou3d_nms_utils"]
ROI_HEAD = ["models.model_utils.model_nms_utils", "models.roi_heads.target_assigner.proposal_target_layer",
            "models.roi_heads.roi_head_template"]
ANCHOR_HEAD = ["models.dense_heads.target_assigner.anchor_generator", "models.dense_heads.target_assigner.atss_target_assigner",
               "models.dense_heads.target_assigner.axis_aligned_target_assigner", "models.dense_heads.anchor_head_template"]
# what models/detectors/detector3d_template.py imports at the top and no fixture reaches: empty packages (a `stubs` of `load`)
DETECTOR_STUBS = {"utils.spconv_utils": {"find_all_spconv_keys": None}, "models.backbones_2d.map_to_bev": {},
                  "models.backbones_3d.pfe": {}, "models.backbones_3d.vfe": {}, "models.dense_heads": {}}


def reference_root():
    """The reference checkout: argv[1], else $PDA_REFERENCE, else $PDA_REFERENCE_ROOT; without one, exit with the docstring
    of the script that runs."""
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PDA_REFERENCE") or os.environ.get("PDA_REFERENCE_ROOT")
    if not root:
        sys.exit(getattr(sys.modules.get("__main__"), "__doc__", None)
                 or "the reference checkout is needed: pass its path, or set PDA_REFERENCE")
    return root


# ---- registration -----------------------------------------------------------------------------------------------------------
def register(name, mod):
    """`mod` as sys.modules[name] and as the attribute of its parent package, if that is registered."""
    sys.modules[name] = mod
    parent, _, leaf = name.rpartition(".")
    if parent in sys.modules:
        setattr(sys.modules[parent], leaf, mod)
    return mod


def package(name, path=None, **attrs):
    """A package of that name: empty, or over the directory `path` (importlib then finds the files in it)."""
    pkg = types.ModuleType(name)
    pkg.__path__ = [path] if path else []
    pkg.__dict__.update(attrs)
    return register(name, pkg)


def module(name, path):
    """The file `path` executed as module `name`; registered first, so that what it imports can import it back."""
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    register(name, m)
    spec.loader.exec_module(m)
    return m


def load(root, prefix, names, stubs=None, real_paths=False):
    """Loads pcdet/<a>/<b>.py of the checkout `root` as <prefix>.a.b for every dotted name 'a.b' of `names`, in that order, and
    returns the modules in that order.  Missing parent packages are registered first: empty ones, or with real_paths=True
    over their directories, so that the reference's own imports find the sibling files that are not stubbed.  stubs:
    {dotted name: a module object, or a dict of attributes for an empty package}, registered before any file runs."""
    pcdet = os.path.join(root, "pcdet")
    if prefix not in sys.modules:
        package(prefix, pcdet)

    def parents(parts):
        for i in range(1, len(parts)):
            name = ".".join([prefix] + parts[:i])
            if name not in sys.modules:
                package(name, os.path.join(pcdet, *parts[:i]) if real_paths else None)

    for dotted, stub in (stubs or {}).items():
        parents(dotted.split("."))
        if isinstance(stub, types.ModuleType):
            register(prefix + "." + dotted, stub)
        else:
            package(prefix + "." + dotted, None, **stub)
    mods = []
    for dotted in names:
        parts = dotted.split(".")
        parents(parts)
        mods.append(module(prefix + "." + dotted, os.path.join(pcdet, *parts) + ".py"))
    return mods


# ---- CPU patches and third-party stubs ----------------------------------------------------------------------------------------
def cpu_torch():
    """The reference allocates with torch.cuda.IntTensor / FloatTensor and moves tensors with .cuda(): the former become the
    CPU constructors, the latter the identity.  The third-party packages its files import at the top and the fixtures never
    reach (SharedArray, skimage, cumm, open3d) become empty modules."""
    torch.cuda.IntTensor, torch.cuda.FloatTensor = torch.IntTensor, torch.FloatTensor
    torch.Tensor.cuda = lambda self, *a, **k: self
    for name in ("SharedArray", "cumm", "open3d", "skimage", "skimage.transform", "skimage.io"):
        register(name, types.ModuleType(name))


def stub_numba():
    """numba: jit / njit / cuda.jit are identity decorators (bare or called), cuda.local.array is np.zeros(..., float32)."""
    ident = lambda *a, **k: (lambda f: f) if not (len(a) == 1 and callable(a[0]) and not k) else a[0]   # noqa: E731
    cuda = types.ModuleType("numba.cuda")
    cuda.jit = ident
    cuda.local = types.SimpleNamespace(array=lambda shape, dtype=None: np.zeros(shape, np.float32))
    cuda.shared = cuda.local
    numba = types.ModuleType("numba")
    numba.jit = numba.njit = ident
    numba.float32 = np.float32
    register("numba", numba)
    register("numba.cuda", cuda)


@contextlib.contextmanager
def precision(dtype):
    """float64: the reference's torch.cuda.FloatTensor allocations and .float() casts give doubles."""
    if dtype == torch.float32:
        yield
        return
    alloc, own = torch.cuda.FloatTensor, torch.Tensor.__dict__.get('float')
    torch.cuda.FloatTensor = torch.DoubleTensor
    torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        yield
    finally:
        torch.cuda.FloatTensor = alloc
        if own is None:
            del torch.Tensor.float
        else:
            torch.Tensor.float = own


# ---- extension stand-ins that several fixtures share ---------------------------------------------------------------------------
def as_np(t):
    """The tensor's memory as an array: a stand-in writes the caller's buffers in place."""
    assert t.device.type == "cpu" and t.is_contiguous()
    return t.detach().numpy()


def np_args(args):
    return [as_np(a) if isinstance(a, torch.Tensor) else a for a in args]


def _c32(x):
    return np.ascontiguousarray(x.detach().numpy(), dtype=np.float32)


def _overlap_bev(boxes_a, boxes_b, ans):
    oracle.boxes_overlap_bev_gpu(boxes_a.numpy(), boxes_b.numpy(), ans.numpy())   # writes through to the tensor


def _nms_gpu(boxes, keep, thresh):
    return oracle.nms_gpu(np.ascontiguousarray(boxes.numpy()), keep.numpy(), float(thresh))


def _points_in_boxes_cpu(points, boxes):
    out = np.zeros((boxes.shape[0], points.shape[0]), np.int32)
    roi_pool_restatement.points_in_boxes_cpu(boxes.numpy().astype(np.float32), points.numpy().astype(np.float32), out)
    return torch.from_numpy(out)


def _points_in_boxes_gpu(points, boxes):
    return torch.from_numpy(stack_sa_restatement.points_in_boxes_gpu(_c32(points), _c32(boxes)))


# the data stages' points_in_boxes_cpu (make_augment_golden, make_frame_stage_golden): float32 rotation, float64 comparisons, the
# margin of the C++ CPU test; not the restatement above, which states the kernels' arithmetic
def points_in_boxes_cpu_np(points, boxes):
    """roiaware_pool3d.cpp check_pt_in_box3d_cpu for every (box, point): (N, num_points) int."""
    pts = np.asarray(points, np.float32)
    out = np.zeros((boxes.shape[0], pts.shape[0]), np.int32)
    for i, b in enumerate(np.asarray(boxes, np.float32)):
        cx, cy, cz, dx, dy, dz, rz = b[:7]
        zin = np.abs(pts[:, 2] - cz).astype(np.float64) <= np.float64(dz) / 2.0
        cosa, sina = np.float32(np.cos(-np.float64(rz))), np.float32(np.sin(-np.float64(rz)))
        sx, sy = pts[:, 0] - cx, pts[:, 1] - cy
        lx = sx * cosa + sy * (-sina)
        ly = sx * sina + sy * cosa
        m = np.float64(np.float32(1e-2))
        inx = np.abs(lx).astype(np.float64) < np.float64(dx) / 2.0 + m
        iny = np.abs(ly).astype(np.float64) < np.float64(dy) / 2.0 + m
        out[i] = (zin & inx & iny).astype(np.int32)
    return out


def extension_stubs(more=()):
    """The stubs argument of `load` for the two compiled packages nearly every model file imports: iou3d_nms_cuda over the C
    oracle (boxes_overlap_bev_gpu, nms_gpu), roiaware_pool3d_utils with points_in_boxes_cpu / points_in_boxes_gpu over the
    numpy restatements.  more: a generator's further entries."""
    stubs = {"ops.roiaware_pool3d.roiaware_pool3d_utils": {"points_in_boxes_cpu": _points_in_boxes_cpu,
                                                           "points_in_boxes_gpu": _points_in_boxes_gpu},
             "ops.iou3d_nms.iou3d_nms_cuda": {"boxes_overlap_bev_gpu": _overlap_bev, "nms_gpu": _nms_gpu}}
    stubs.update(more)
    return stubs


def pointnet2_batch_stub():
    """pointnet2_batch_cuda: every entry point passes its arrays to the C oracle's function of the same name."""
    stub = types.ModuleType("pointnet2_batch_cuda")
    for name in ("ball_query_wrapper", "ball_query_dilated_wrapper", "group_points_wrapper", "group_points_grad_wrapper",
                 "gather_points_wrapper", "gather_points_grad_wrapper", "farthest_point_sampling_wrapper",
                 "furthest_point_sampling_with_dist_wrapper", "three_nn_wrapper", "three_interpolate_wrapper",
                 "three_interpolate_grad_wrapper"):
        setattr(stub, name, (lambda fn: lambda *args: fn(*np_args(args)))(getattr(oracle, name)))
    return stub


# ---- small helpers ------------------------------------------------------------------------------------------------------------
def q(x, step=256.0):
    """Values on the 1 / step grid, as float32: compressible coordinates."""
    return (np.round(np.asarray(x, np.float64) * step) / step).astype(np.float32)


def randomise(module, rng):
    """BatchNorm weights, biases and running statistics away from their initial values, so that each of them matters."""
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    for m in module.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            with torch.no_grad():
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)


def state(module, prefix, out):
    for k, v in module.state_dict().items():
        out[prefix + "sd." + k] = v.detach().numpy().copy()


def shapes(module, prefix=""):
    return [[prefix + k, list(v.shape)] for k, v in module.state_dict().items()]


def model_yaml(root, name):
    """tools/cfgs/<name> of the checkout, parsed."""
    with open(os.path.join(root, "tools", "cfgs", *name.split("/"))) as f:
        return yaml.safe_load(f)


def second_settings():
    """second_state_dict.json: the reduced SECONDNet the two-stage state-dict fixtures are built on."""
    with open(os.path.join(HERE, "second_state_dict.json")) as f:
        return json.load(f)


def write_state_dict(name, out):
    path = os.path.join(HERE, name)
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print(path, {k: len(v) for k, v in out.items()})
