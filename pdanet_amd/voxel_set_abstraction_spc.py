"""The keypoint encoder of PV-RCNN++ (pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py:45-121, :206-225, :305-320):
SAMPLE_METHOD SPC -- sample_points_with_roi followed by sector_fps -- and FILTER_NEIGHBOR_WITH_ROI, as a subclass of
voxel_set_abstraction.VoxelSetAbstraction over the hooks that class names; its layers come from
vector_pool_modules.build_local_aggregation_module (StackSAModuleMSG or VectorPoolAggregationModuleMSG).

The reference cuts the batch into scenes, builds an N x M distance matrix per scene and per source (in parts of
NUM_POINTS_OF_EACH_SAMPLE_PART rows) and loops over the sectors in Python with an .item() in each.  Here

  sample_points_with_roi   ONE launch of pda_roi_point_filter (csrc/spc_sample.hip) over the stacked batch: the mask and, when
                           sectors are asked for, the key scene * (num_sectors + 1) + sector of every point.  No N x M tensor
                           exists, so NUM_POINTS_OF_EACH_SAMPLE_PART has nothing to cut and is not read.
  sector_fps               a stable sort of the keys puts the points of every (scene, sector) next to each other in their
                           original order (the points of no sector go to the end); an index_add counts them; ONE host read
                           brings the B x (num_sectors + 1) counts over; the quotas min(cnt, ceil(cnt / n_kept *
                           NUM_KEYPOINTS)) are the reference's own Python float expression on the host; ONE
                           stack_farthest_point_sample launch samples every non-empty segment.  A scene without a sectored
                           point contributes its first point (the reference's rule for a scene whose filter keeps nothing).
  keypoints                ragged, (N1 + N2 + ..., 4), sector-major within a scene, as the reference concatenates them.
  FILTER_NEIGHBOR_WITH_ROI the mask of one launch per source, then nonzero / index_select; autograd carries the feature
                           gradient through the index_select.  ONE host read per filtered source (the size of nonzero's result).
                           A scene that keeps no row of a source has the count 0 there: the three-NN and vector-pool kernels
                           find no neighbour and its pooled features are zeros, as in the reference.

Host reads per forward: one for the keypoints, one per filtered source, plus those of the layers themselves.
The points of every source must be ordered by scene.  RoIs are read as they are: every row of `rois` takes part, zero rows
included, as in the reference."""
import math

import torch

from . import pointnet2_stack_utils
from . import vector_pool_modules
from .pointnet2_batch_cuda import F32, I32, _call, _chk
from .voxel_set_abstraction import VoxelSetAbstraction, scene_counts
from .voxel_utils import get_voxel_centers


def sample_points_with_roi(rois, points, point_cnt, sample_radius_with_roi, num_sectors=0):
    """rois (B, M, 7 + C), points (N, 3) ordered by scene, point_cnt (B) int32 on the device -> mask (N) uint8: the point lies
    nearer to its nearest RoI centre (the lowest index among equals) than that RoI's half diagonal + sample_radius_with_roi;
    and keys (N) int32 = scene * (num_sectors + 1) + sector when num_sectors > 0 (else None): the sector of sector_fps for a
    kept point, num_sectors for one that is not kept; a row past the sum of point_cnt keeps mask 0 and the key B (num_sectors + 1)."""
    points, rois = points.contiguous(), rois.contiguous()
    N, (B, M) = points.shape[0], rois.shape[:2]
    if point_cnt.shape[0] != B:
        raise ValueError("sample_points_with_roi: %d counts for %d scenes of RoIs" % (point_cnt.shape[0], B))
    mask = torch.zeros((N,), dtype=torch.uint8, device=points.device)
    # rows past the sum of the counts belong to no scene: they keep the key B (num_sectors + 1), which sector_fps refuses
    keys = torch.full((N,), B * (num_sectors + 1), dtype=I32, device=points.device) if num_sectors > 0 else None
    if M == 0 and keys is not None:                     # nothing is kept: every point carries its scene's last key
        scene = torch.repeat_interleave(torch.arange(B + 1, device=points.device),
                                        torch.cat((point_cnt.long(), (N - point_cnt.sum()).clamp(min=0).view(1))), output_size=N)
        keys.copy_(torch.where(scene < B, scene * (num_sectors + 1) + num_sectors, scene * (num_sectors + 1)))
    _call("pda_roi_point_filter", points, _chk(points, "points", F32), _chk(point_cnt, "point_cnt", I32), _chk(rois, "rois", F32),
          float(sample_radius_with_roi), mask.data_ptr(), keys.data_ptr() if keys is not None else None, N, B, M, rois.shape[2],
          int(num_sectors))
    return mask, keys


def sector_quotas(counts, kept, num_sampled_points):
    """counts[k] points in sector k of one scene, kept of them passed the filter -> the samples sector_fps asks of each sector
    (voxel_set_abstraction.py:96-103, the reference's float expression); 0 for an empty sector."""
    return [min(c, math.ceil(c / kept * num_sampled_points)) if c > 0 else 0 for c in counts]


def sector_fps(points, mask, keys, batch_size, num_sampled_points, num_sectors):
    """points (N, 3) ordered by scene with the mask and keys of sample_points_with_roi -> rows of `points` (K1 + K2 + ...)
    int64, sector-major within a scene, and the keypoints per scene as a list.  One host read."""
    S = num_sectors + 1
    keys = keys.long()
    tally = torch.zeros((batch_size * S + 1, 2), dtype=torch.int64, device=points.device)     # the last row: points of no scene
    tally.index_add_(0, keys, torch.stack((torch.ones_like(keys), mask.long()), dim=1))
    # the points of no sector (not kept, or the clamped index num_sectors) behind everything else
    order = torch.sort(torch.where(keys % S == num_sectors, batch_size * S, keys), stable=True)[1]           # (no scene: there already)
    tally = tally.tolist()                                                                       # the one host read
    if tally[-1][0]:
        raise ValueError("sector_fps: %d points lie past the per-scene counts the keys were made with" % tally[-1][0])
    tally = [tally[b * S:(b + 1) * S] for b in range(batch_size)]
    seg_cnt, seg_quota, pieces, start = [], [], [], 0
    for scene in tally:
        counts, kept = [c for c, _ in scene[:num_sectors]], sum(k for _, k in scene)
        quotas = sector_quotas(counts, kept, num_sampled_points) if kept > 0 else []
        seg_cnt += [c for c in counts if c > 0]
        seg_quota += [q for q in quotas if q > 0]
        pieces.append((sum(quotas), start))
        if sum(c for c, _ in scene) < 1:
            raise ValueError("VoxelSetAbstraction: a scene without points")
        start += sum(c for c, _ in scene)
    rows = None
    if seg_cnt:
        sectored = points[order[:sum(seg_cnt)]].contiguous()
        cnt = torch.tensor(seg_cnt, dtype=I32).to(points.device, non_blocking=True)
        rows = order[pointnet2_stack_utils.stack_farthest_point_sample(sectored, cnt, seg_quota).long()]
    out, done, per_scene = [], 0, []
    for n, first_row in pieces:
        if n > 0:
            out.append(rows[done:done + n])
            done += n
        else:
            out.append(torch.full((1,), first_row, dtype=torch.int64, device=points.device))
        per_scene.append(max(n, 1))
    return torch.cat(out), per_scene


class VoxelSetAbstractionSPC(VoxelSetAbstraction):
    SAMPLE_METHODS = ('FPS', 'SPC')
    NEIGHBOR_FILTER = True
    build_local_aggregation_module = staticmethod(vector_pool_modules.build_local_aggregation_module)

    def keypoints_and_counts(self, batch_dict):
        if self.model_cfg['SAMPLE_METHOD'] != 'SPC':
            return super().keypoints_and_counts(batch_dict)
        batch_size = batch_dict['batch_size']
        if self.model_cfg['POINT_SOURCE'] == 'raw_points':
            src_points, batch_column = batch_dict['points'][:, 1:4], batch_dict['points'][:, 0]
        else:
            src_points = get_voxel_centers(batch_dict['voxel_coords'][:, 1:4], downsample_times=1, voxel_size=self.voxel_size,
                                           point_cloud_range=self.point_cloud_range)
            batch_column = batch_dict['voxel_coords'][:, 0]
        src_points = src_points.float().contiguous()
        point_cnt = scene_counts(batch_column, batch_size)
        spc = self.model_cfg['SPC_SAMPLING']
        mask, keys = sample_points_with_roi(batch_dict['rois'], src_points, point_cnt, spc['SAMPLE_RADIUS_WITH_ROI'],
                                            num_sectors=spc['NUM_SECTORS'])
        rows, per_scene = sector_fps(src_points, mask, keys, batch_size, self.model_cfg['NUM_KEYPOINTS'], spc['NUM_SECTORS'])
        cnt = torch.tensor(per_scene, dtype=torch.int32).to(src_points.device, non_blocking=True)
        bs_idx = torch.repeat_interleave(torch.arange(batch_size, device=rows.device), cnt.long(), output_size=rows.shape[0])
        return torch.cat((bs_idx.float().view(-1, 1), src_points[rows]), dim=1), cnt

    def source_rows(self, src_name, xyz, xyz_features, xyz_bs_idxs, batch_dict):
        cfg = self.model_cfg['SA_LAYER'][src_name]
        if not cfg.get('FILTER_NEIGHBOR_WITH_ROI', False):
            return xyz, xyz_features, xyz_bs_idxs
        mask, _ = sample_points_with_roi(batch_dict['rois'], xyz.float(), scene_counts(xyz_bs_idxs, batch_dict['batch_size']),
                                         cfg['RADIUS_OF_NEIGHBOR_WITH_ROI'])
        rows = torch.nonzero(mask).view(-1)                                                      # the one host read
        return xyz.index_select(0, rows), xyz_features.index_select(0, rows), xyz_bs_idxs.index_select(0, rows)
