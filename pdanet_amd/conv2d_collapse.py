"""Conv2DCollapse (pcdet/models/backbones_2d/map_to_bev/conv2d_collapse.py): voxel_features (B, C, Z, Y, X) -> spatial_features
(B, C, Y, X) by folding the heights into the channels and one BasicBlock2D (`block`, a torch 1x1 convolution over C * Z
channels).  Folding that K = C * Z contraction into the sampling kernel, so that the voxel tensor disappears too, is the
next lever and not done here."""
import torch.nn as nn

from .image_vfe import BasicBlock2D


class Conv2DCollapse(nn.Module):
    def __init__(self, model_cfg, grid_size):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_heights = int(grid_size[-1])
        self.num_bev_features = model_cfg['NUM_BEV_FEATURES']
        self.block = BasicBlock2D(in_channels=self.num_bev_features * self.num_heights, out_channels=self.num_bev_features,
                                  **dict(model_cfg['ARGS']))

    def forward(self, batch_dict):
        voxel_features = batch_dict["voxel_features"]
        batch_dict["spatial_features"] = self.block(voxel_features.flatten(start_dim=1, end_dim=2))
        return batch_dict
