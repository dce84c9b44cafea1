"""Convolutional Neural Operator in 1-D (reference models/CNO1d.py): the module tree of models/cno_nd.py bound to
nn.Conv1d, nn.BatchNorm1d and rpde.ops conv1d_k3, batchnorm1d, cno_act1d.  Each class names the rank and the classes of
this module that it builds its children from."""
from models import cno_nd

_ND = cno_nd.RANK[1]


class CNO_LReLu(cno_nd.CNO_LReLu):
    nd = _ND


class CNOBlock(cno_nd.CNOBlock):
    nd, CNO_LReLu = _ND, CNO_LReLu


class LiftProjectBlock(cno_nd.LiftProjectBlock):
    nd, CNOBlock = _ND, CNOBlock


class ResidualBlock(cno_nd.ResidualBlock):
    nd, CNO_LReLu = _ND, CNO_LReLu


class ResNet(cno_nd.ResNet):
    ResidualBlock = ResidualBlock


class CNO1d(cno_nd.CNO):
    """in_dim / out_dim channels on `size` points; N_layers down- and up-sampling levels, N_res residual blocks per
    level and N_res_neck in the neck; level i has channel_multiplier 2^(i-1) channels on size / 2^i points.  Inputs of
    another length are resampled by the first activation (F.interpolate(size=...) in the reference does the same)."""
    LiftProjectBlock, CNOBlock, ResNet = LiftProjectBlock, CNOBlock, ResNet
