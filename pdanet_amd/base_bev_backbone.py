"""BaseBEVBackbone (pcdet/models/backbones_2d/base_bev_backbone.py) in plain torch with the reference's constructor
signature, config keys (LAYER_NUMS, LAYER_STRIDES, NUM_FILTERS, UPSAMPLE_STRIDES, NUM_UPSAMPLE_FILTERS) and state-dict
keys (blocks.{i}.{j}.*, deblocks.{i}.{j}.*).  Its convolutions are library calls and are not tuned here."""
import torch
import torch.nn as nn


def _bn(channels):
    return nn.BatchNorm2d(channels, eps=1e-3, momentum=0.01)


def _block(c_in, c_out, stride, extra_layers):
    layers = [nn.ZeroPad2d(1), nn.Conv2d(c_in, c_out, kernel_size=3, stride=stride, padding=0, bias=False), _bn(c_out), nn.ReLU()]
    for _ in range(extra_layers):
        layers += [nn.Conv2d(c_out, c_out, kernel_size=3, padding=1, bias=False), _bn(c_out), nn.ReLU()]
    return nn.Sequential(*layers)


def _deblock(c_in, c_out, stride):
    if stride >= 1:
        conv = nn.ConvTranspose2d(c_in, c_out, stride, stride=stride, bias=False)
    else:                                   # a fractional stride down-samples by its reciprocal
        down = int(round(1 / stride))
        conv = nn.Conv2d(c_in, c_out, down, stride=down, bias=False)
    return nn.Sequential(conv, _bn(c_out), nn.ReLU())


class BaseBEVBackbone(nn.Module):
    def __init__(self, model_cfg, input_channels):
        super().__init__()
        self.model_cfg = model_cfg
        layer_nums = layer_strides = num_filters = []
        if model_cfg.get('LAYER_NUMS', None) is not None:
            layer_nums, layer_strides, num_filters = model_cfg['LAYER_NUMS'], model_cfg['LAYER_STRIDES'], model_cfg['NUM_FILTERS']
            assert len(layer_nums) == len(layer_strides) == len(num_filters)
        upsample_strides = num_upsample_filters = []
        if model_cfg.get('UPSAMPLE_STRIDES', None) is not None:
            upsample_strides, num_upsample_filters = model_cfg['UPSAMPLE_STRIDES'], model_cfg['NUM_UPSAMPLE_FILTERS']
            assert len(upsample_strides) == len(num_upsample_filters)
        levels = len(layer_nums)
        c_in = [input_channels] + list(num_filters[:-1])
        self.blocks = nn.ModuleList(_block(c_in[i], num_filters[i], layer_strides[i], layer_nums[i]) for i in range(levels))
        self.deblocks = nn.ModuleList()
        if len(upsample_strides) > 0:
            for i in range(levels):
                self.deblocks.append(_deblock(num_filters[i], num_upsample_filters[i], upsample_strides[i]))
        c_out = sum(num_upsample_filters)
        if len(upsample_strides) > levels:
            self.deblocks.append(_deblock(c_out, c_out, upsample_strides[-1]))
        self.num_bev_features = c_out

    def forward(self, data_dict):
        """data_dict['spatial_features'] (B, C, ny, nx) -> 'spatial_features_2d'."""
        ups = []
        x = data_dict['spatial_features']
        for i, block in enumerate(self.blocks):
            x = block(x)
            ups.append(self.deblocks[i](x) if len(self.deblocks) > 0 else x)
        if len(ups) > 1:
            x = torch.cat(ups, dim=1)
        elif len(ups) == 1:
            x = ups[0]
        if len(self.deblocks) > len(self.blocks):
            x = self.deblocks[-1](x)
        data_dict['spatial_features_2d'] = x
        return data_dict
