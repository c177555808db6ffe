"""DDNDeepLabV3 (pcdet/models/backbones_3d/vfe/image_vfe_modules/ffn/ddn): the depth distribution network of CaDDN, in plain
torch.  The reference takes torchvision's deeplabv3_resnet50 / deeplabv3_resnet101; torchvision is not a dependency here, so
the same module tree is built under `model.` with the same state-dict keys, and the COCO checkpoint
(deeplabv3_resnet101_coco-586e9e4e.pth) and a reference CaDDN checkpoint both load:

  model.backbone    conv1, bn1, relu, maxpool, layer1..4 of Bottlenecks [3, 4, 6, 3] / [3, 4, 23, 3]; the stride sits on conv2, a
                    downsample.0/1 in each layer's first block, layer3 and layer4 dilated instead of strided (output stride 8)
  model.classifier  0 = ASPP (convs.0 1x1; convs.1..3 3x3 with dilations 12 / 24 / 36; convs.4 = pool, conv .1, BN .2;
                    project.0/1 and Dropout 0.5), 1 = 3x3 conv, 2 = BN, 4 = 1x1 conv to num_classes with bias
There is no aux_classifier (aux_loss is out of scope).

forward follows ddn_template.py: the features of `feat_extract_layer`, the logits resized bilinearly to the feature size;
`preprocess` runs only with a pretrained_path (NaN mask, ImageNet mean / std, masked pixels 0).  pretrained_path is loaded
through filter_pretrained_dict if the file exists; a missing file raises FileNotFoundError -- nothing is ever downloaded."""
import os
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

LAYERS = {'ResNet50': [3, 4, 6, 3], 'ResNet101': [3, 4, 23, 3]}


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, dilation=1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + identity)


class ResNetBody(nn.ModuleDict):
    """torchvision's IntermediateLayerGetter over a ResNet with replace_stride_with_dilation = [False, True, True]: the
    modules up to layer4 in order, the outputs of `return_layers` under their new names."""

    def __init__(self, layers, return_layers):
        self.inplanes, self.dilation = 64, 1
        mods = OrderedDict()
        mods['conv1'] = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        mods['bn1'] = nn.BatchNorm2d(64)
        mods['relu'] = nn.ReLU(inplace=True)
        mods['maxpool'] = nn.MaxPool2d(3, stride=2, padding=1)
        for n, (planes, blocks, stride, dilate) in enumerate(zip((64, 128, 256, 512), layers, (1, 2, 2, 2),
                                                                 (False, False, True, True))):
            mods['layer%d' % (n + 1)] = self._make_layer(planes, blocks, stride, dilate)
        super().__init__(mods)
        self.return_layers = dict(return_layers)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')

    def _make_layer(self, planes, blocks, stride, dilate):
        previous = self.dilation
        if dilate:
            self.dilation *= stride
            stride = 1
        downsample = None
        if stride != 1 or self.inplanes != planes * Bottleneck.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * Bottleneck.expansion, 1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * Bottleneck.expansion))
        layers = [Bottleneck(self.inplanes, planes, stride, downsample, previous)]
        self.inplanes = planes * Bottleneck.expansion
        layers += [Bottleneck(self.inplanes, planes, dilation=self.dilation) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def forward(self, x):
        out = OrderedDict()
        for name, module in self.items():
            x = module(x)
            if name in self.return_layers:
                out[self.return_layers[name]] = x
        return out


class ASPPPooling(nn.Sequential):
    def __init__(self, in_channels, out_channels):
        super().__init__(nn.AdaptiveAvgPool2d(1), nn.Conv2d(in_channels, out_channels, 1, bias=False),
                         nn.BatchNorm2d(out_channels), nn.ReLU())

    def forward(self, x):
        size = x.shape[-2:]
        for mod in self:
            x = mod(x)
        return F.interpolate(x, size=size, mode='bilinear', align_corners=False)


class ASPP(nn.Module):
    def __init__(self, in_channels, atrous_rates=(12, 24, 36), out_channels=256):
        super().__init__()
        convs = [nn.Sequential(nn.Conv2d(in_channels, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU())]
        convs += [nn.Sequential(nn.Conv2d(in_channels, out_channels, 3, padding=r, dilation=r, bias=False),
                                nn.BatchNorm2d(out_channels), nn.ReLU()) for r in atrous_rates]
        convs.append(ASPPPooling(in_channels, out_channels))
        self.convs = nn.ModuleList(convs)
        self.project = nn.Sequential(nn.Conv2d(len(convs) * out_channels, out_channels, 1, bias=False),
                                     nn.BatchNorm2d(out_channels), nn.ReLU(), nn.Dropout(0.5))

    def forward(self, x):
        return self.project(torch.cat([conv(x) for conv in self.convs], dim=1))


class DeepLabV3(nn.Module):
    def __init__(self, layers, num_classes, feat_extract_layer):
        super().__init__()
        self.backbone = ResNetBody(layers, {feat_extract_layer: 'features', 'layer4': 'out'})
        self.classifier = nn.Sequential(ASPP(2048), nn.Conv2d(256, 256, 3, padding=1, bias=False), nn.BatchNorm2d(256), nn.ReLU(),
                                        nn.Conv2d(256, num_classes, 1))
        self.aux_classifier = None


class DDNDeepLabV3(nn.Module):
    def __init__(self, backbone_name, feat_extract_layer, num_classes, pretrained_path=None, aux_loss=None):
        super().__init__()
        if backbone_name not in LAYERS:
            raise NotImplementedError("DDN.BACKBONE_NAME %r (ResNet50, ResNet101)" % (backbone_name,))
        if aux_loss:
            raise NotImplementedError("DDN aux_loss")
        if feat_extract_layer not in ('layer1', 'layer2', 'layer3'):
            raise NotImplementedError("DDN feat_extract_layer %r (layer1, layer2, layer3)" % (feat_extract_layer,))
        self.num_classes, self.pretrained_path, self.aux_loss = num_classes, pretrained_path, aux_loss
        self.pretrained = pretrained_path is not None
        if self.pretrained and not os.path.exists(pretrained_path):
            raise FileNotFoundError("DDN pretrained_path %r does not exist (nothing is downloaded: fetch torchvision's "
                                    "deeplabv3 COCO checkpoint yourself, or set pretrained_path to None)" % (pretrained_path,))
        if self.pretrained:
            self.norm_mean = torch.Tensor([0.485, 0.456, 0.406])
            self.norm_std = torch.Tensor([0.229, 0.224, 0.225])
        self.feat_extract_layer = feat_extract_layer
        self.model = DeepLabV3(LAYERS[backbone_name], num_classes, feat_extract_layer)
        if self.pretrained:
            model_dict = self.model.state_dict()
            pretrained_dict = self.filter_pretrained_dict(model_dict, torch.load(pretrained_path, map_location='cpu'))
            model_dict.update(pretrained_dict)
            self.model.load_state_dict(model_dict)

    @staticmethod
    def filter_pretrained_dict(model_dict, pretrained_dict):
        """Drops the aux classifier's weights when the model has none, and the last convolution when the class counts differ."""
        if "aux_classifier.0.weight" in pretrained_dict and "aux_classifier.0.weight" not in model_dict:
            pretrained_dict = {k: v for k, v in pretrained_dict.items() if "aux_classifier" not in k}
        if model_dict["classifier.4.weight"].shape[0] != pretrained_dict["classifier.4.weight"].shape[0]:
            pretrained_dict = {k: v for k, v in pretrained_dict.items() if k not in ("classifier.4.weight", "classifier.4.bias")}
        return pretrained_dict

    def preprocess(self, images):
        if not self.pretrained:
            return images
        mask = torch.isnan(images)
        mean = self.norm_mean.to(images).view(1, 3, 1, 1)
        std = self.norm_std.to(images).view(1, 3, 1, 1)
        return torch.where(mask, torch.zeros_like(images), (images - mean) / std)

    def forward(self, images):
        """images (N, 3, H, W) -> {'features': (N, C, Hf, Wf) of feat_extract_layer, 'logits': (N, num_classes, Hf, Wf)}."""
        features = self.model.backbone(self.preprocess(images))
        result = OrderedDict()
        result['features'] = features['features']
        logits = self.model.classifier(features['out'])
        result['logits'] = F.interpolate(logits, size=features['features'].shape[-2:], mode='bilinear', align_corners=False)
        return result
