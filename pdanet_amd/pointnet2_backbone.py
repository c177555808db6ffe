"""PointNet2MSG (pcdet/models/backbones_3d/pointnet2_backbone.py:9-94): the PointNet++ encoder-decoder of PointRCNN, under
the reference's module names (SA_modules, FP_modules) and state-dict keys.

`points` (B * N, 1 + 3 + C) [bs_idx, x, y, z, ...] must be scene-major with equally many rows per scene (the reference asserts
the same); the per-scene count comes from the shape, where the reference counts each scene's rows on the host.  Nothing is
read on the host.  PointNet2Backbone (the stack variant) is not built: the reference asserts it off."""
import torch
import torch.nn as nn

from . import pointnet2_modules


class PointNet2MSG(nn.Module):
    def __init__(self, model_cfg, input_channels, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        sa_cfg = model_cfg['SA_CONFIG']
        self.SA_modules = nn.ModuleList()
        channel_in = input_channels - 3
        skip_channel_list = [input_channels - 3]
        channel_out = channel_in
        for k in range(len(sa_cfg['NPOINTS'])):
            mlps = [[channel_in] + list(spec) for spec in sa_cfg['MLPS'][k]]
            channel_out = sum(spec[-1] for spec in mlps)
            self.SA_modules.append(pointnet2_modules.PointnetSAModuleMSG(
                npoint=sa_cfg['NPOINTS'][k], radii=sa_cfg['RADIUS'][k], nsamples=sa_cfg['NSAMPLE'][k], mlps=mlps,
                use_xyz=sa_cfg.get('USE_XYZ', True)))
            skip_channel_list.append(channel_out)
            channel_in = channel_out

        fp_mlps = model_cfg['FP_MLPS']
        self.FP_modules = nn.ModuleList()
        for k in range(len(fp_mlps)):
            pre_channel = fp_mlps[k + 1][-1] if k + 1 < len(fp_mlps) else channel_out
            self.FP_modules.append(pointnet2_modules.PointnetFPModule(mlp=[pre_channel + skip_channel_list[k]] + list(fp_mlps[k])))
        self.num_point_features = fp_mlps[0][-1]

    def forward(self, batch_dict):
        """batch_size, points (B * N, 4 + C) -> point_features (B * N, C'), point_coords (B * N, 4) [bs_idx, x, y, z]."""
        batch_size = batch_dict['batch_size']
        points = batch_dict['points']
        if points.shape[0] % batch_size != 0:
            raise ValueError("PointNet2MSG needs equally many points per scene, got %d rows for %d scenes"
                             % (points.shape[0], batch_size))
        batch_idx = points[:, 0]
        xyz = points[:, 1:4].contiguous().view(batch_size, -1, 3)
        features = None
        if points.shape[-1] > 4:
            features = points[:, 4:].contiguous().view(batch_size, -1, points.shape[-1] - 4).permute(0, 2, 1).contiguous()

        l_xyz, l_features = [xyz], [features]
        for i in range(len(self.SA_modules)):
            li_xyz, li_features = self.SA_modules[i](l_xyz[i], l_features[i])
            l_xyz.append(li_xyz)
            l_features.append(li_features)
        for i in range(-1, -(len(self.FP_modules) + 1), -1):
            l_features[i - 1] = self.FP_modules[i](l_xyz[i - 1], l_xyz[i], l_features[i - 1], l_features[i])   # (B, C, N)

        point_features = l_features[0].permute(0, 2, 1).contiguous()                                            # (B, N, C)
        batch_dict['point_features'] = point_features.view(-1, point_features.shape[-1])
        batch_dict['point_coords'] = torch.cat((batch_idx[:, None].float(), l_xyz[0].view(-1, 3)), dim=1)
        return batch_dict
