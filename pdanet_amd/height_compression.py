"""HeightCompression (pcdet/models/backbones_2d/map_to_bev/height_compression.py): the encoded sparse tensor made dense
and its depth folded into the channels."""
import torch.nn as nn

from .config import field


class HeightCompression(nn.Module):
    def __init__(self, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_bev_features = field(model_cfg, 'NUM_BEV_FEATURES')

    def forward(self, batch_dict):
        """encoded_spconv_tensor -> spatial_features (B, C * D, H, W), spatial_features_stride.  A padded tensor scatters its
        live rows only (dense() hands num_active to the scatter as its device count); voxel_status stays in the batch."""
        spatial_features = batch_dict['encoded_spconv_tensor'].dense()
        N, C, D, H, W = spatial_features.shape
        batch_dict['spatial_features'] = spatial_features.view(N, C * D, H, W)
        batch_dict['spatial_features_stride'] = batch_dict['encoded_spconv_tensor_stride']
        return batch_dict
