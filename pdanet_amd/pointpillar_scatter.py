"""PointPillarScatter (pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py) on the device: pillar features to the
dense BEV map in one fill and one launch for the whole batch (csrc/pillar.hip pillar_scatter_kernel), where the
reference loops over scenes behind coords[:, 0].max().item().

The forward is a copy and therefore bit-exact; the backward is the gather of the same cells (no atomics).  The cell index
is the reference's c1 + c2 * nx + c3 of voxel_coords (b, z, y, x).  A row whose batch index is outside [0, B) or whose
cell is outside the grid is skipped.  Two rows on one cell are OUTSIDE THE CONTRACT (DynamicPillarVFE emits each cell
once): which row a cell then keeps is not defined, and the backward hands the cell's gradient to both.

Two forms: `pillar_scatter(features, coords, B, ny, nx)` takes the sliced tensors of DynamicPillarVFE's batch_dict;
`pillar_scatter(..., count=index.counts[1:2])` takes the operators' padded form (dyn_voxel_utils: features and coords
padded to n rows plus the device count of live pillars), for a caller that wants no host read."""
import torch
import torch.nn as nn

from .config import field
from .pointnet2_batch_cuda import F32, I32, _call, _chk


def _check(features, coords, count):
    _chk(features, "pillar_features", F32)
    _chk(coords, "voxel_coords", I32)
    if features.dim() != 2 or coords.dim() != 2 or coords.shape[1] != 4 or coords.shape[0] < features.shape[0]:
        raise ValueError("pillar_features must be (n, C) and voxel_coords (>= n, 4), got %s and %s"
                         % (tuple(features.shape), tuple(coords.shape)))
    if count is not None:
        _chk(count, "count", I32)
        if count.numel() != 1:
            raise ValueError("count must hold one int32")


class _Scatter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, coords, count, B, ny, nx):
        n, C = features.shape
        out = torch.zeros((B, C, ny, nx), dtype=F32, device=features.device)          # the one fill
        _call("pda_pillar_scatter_fwd", features, features.data_ptr(), coords.data_ptr(),
              None if count is None else count.data_ptr(), n, C, B, ny, nx, out.data_ptr())
        ctx.coords, ctx.count, ctx.dims = coords, count, (n, C, B, ny, nx)
        return out

    @staticmethod
    def backward(ctx, grad):
        n, C, B, ny, nx = ctx.dims
        grad = grad.contiguous()
        g = torch.empty((n, C), dtype=F32, device=grad.device)
        if B * ny * nx == 0:
            return g.zero_(), None, None, None, None, None
        _call("pda_pillar_scatter_bwd", grad, _chk(grad, "grad", F32), ctx.coords.data_ptr(),
              None if ctx.count is None else ctx.count.data_ptr(), n, C, B, ny, nx, g.data_ptr())
        return g, None, None, None, None, None


def pillar_scatter(features, coords, batch_size, ny, nx, count=None):
    """features (n, C) float32, coords (>= n, 4) int32 (b, z, y, x), count None or a device int32 (rows from it on are
    padding) -> (batch_size, C, ny, nx), zero where no pillar lies.  Differentiable in features.  No host read."""
    _check(features, coords, count)
    return _Scatter.apply(features, coords, count, int(batch_size), int(ny), int(nx))


class PointPillarScatter(nn.Module):
    def __init__(self, model_cfg, grid_size, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_bev_features = field(model_cfg, "NUM_BEV_FEATURES")
        self.nx, self.ny, self.nz = (int(v) for v in grid_size)
        assert self.nz == 1

    def forward(self, batch_dict, **kwargs):
        """batch_dict: pillar_features (n, C), voxel_coords (n, 4) int32 (b, z, y, x), batch_size (when the key is absent
        it is read from the coordinates as the reference does: one host read) -> spatial_features (B, C * nz, ny, nx).
        With 'pillar_count' (a device int32, the padded form) the rows from it on are ignored."""
        features, coords = batch_dict['pillar_features'], batch_dict['voxel_coords']
        if 'batch_size' in batch_dict:
            batch_size = int(batch_dict['batch_size'])
        else:
            batch_size = int(coords[:, 0].max().item()) + 1 if coords.shape[0] else 0
        coords = coords if coords.dtype == I32 else coords.to(I32)
        batch_dict['spatial_features'] = pillar_scatter(features.contiguous(), coords.contiguous(), batch_size, self.ny, self.nx,
                                                        count=batch_dict.get('pillar_count'))
        return batch_dict
