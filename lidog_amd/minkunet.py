"""MinkUNet34 / MinkUNet34BEV wiring, generic over the operator backend.

Mirrors the module names, parameter names (state_dict keys) and call order of
the reference models so reference checkpoints load unchanged:

  MinkUNet34BEV  utils/models/minkunet_bev.py:9-156 (layers), :302-399 (forward), :445-447
  MinkUNet34     utils/models/minkunet.py:23-95 (layers), :97-158 (forward), :171-174
  MinkUNet34IBN  utils/models/minkunet_ibn.py:9-50 (IBNBlock), :53-206, :209-211; _make_layer and
                 weight_initialization of utils/models/resnet_old.py:57-97
  MinkUNet34Robust  utils/models/minkunet_robustnet.py:9-53 (RobustBlock), :56-224 (layers, forward), :227-230
  BasicBlock     MinkowskiEngine.modules.resnet_block (evidence: utils/models/resnet_block.py:8-56)

``make_models(ME, Encoder2D, sparse2super)`` binds the wiring to an operator
module exposing the MinkowskiEngine names of SURVEY.md 8(b).  The product binds
it to ``lidog_amd.me`` (HIP kernels) at the bottom of ``lidog_amd/__init__.py``;
the test-suite binds the same wiring to the CPU oracle, after proving in the
build container that this wiring equals the reference classes bit for bit.
"""
import types

import torch.nn as nn

# (PLANES, LAYERS) of MinkUNet34 (minkunet_bev.py:14,445-447)
PLANES = (32, 64, 128, 256, 256, 128, 96, 96)
LAYERS34 = (2, 3, 4, 6, 2, 2, 2, 2)
INIT_DIM = 32
# encoder stage i: conv{i}p{s}s2 / bn{i} / block{i};  decoder stage j: convtr{j}p{s}s2 / bntr{j} / block{j+1}
_ENC = [(1, 1), (2, 2), (3, 4), (4, 8)]
_DEC = [(4, 16), (5, 8), (6, 4), (7, 2)]
BEV_LEVEL_CHANNELS = {"block8": 96, "block7": 96, "block6": 128, "bottle": 256}


def make_models(ME, Encoder2D=None, sparse2super=None):
    BasicBlock = ME.modules.resnet_block.BasicBlock
    _fused = getattr(ME, "bn_relu", None)  # optional backend fast path: BN + ReLU in one kernel
    _conv_bn = getattr(ME, "conv_bn", None)
    _trunk_exec = getattr(ME, "trunk_forward", None)  # optional: the whole trunk as one launch sequence
    _ibn = getattr(ME, "ibn_relu", None)  # optional: ReLU(BN(x)) | ReLU(IN(x)) in one pass each way

    class IBNBlock(nn.Module):
        """minkunet_ibn.py:9-50: conv1 -> (BatchNorm | InstanceNorm of the same output) -> cat -> ReLU -> conv2 (2 planes
        -> planes) -> norm2 -> += downsample(x) -> ReLU"""
        expansion = 1

        def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, bn_momentum=0.1, dimension=-1):
            super().__init__()
            assert dimension > 0
            self.conv1 = ME.MinkowskiConvolution(inplanes, planes, kernel_size=3, stride=stride, dilation=dilation,
                                                 dimension=dimension)
            self.bn_norm1 = ME.MinkowskiBatchNorm(planes, momentum=bn_momentum)
            self.in_norm1 = ME.MinkowskiInstanceNorm(planes)
            self.conv2 = ME.MinkowskiConvolution(planes * 2, planes, kernel_size=3, stride=1, dilation=dilation,
                                                 dimension=dimension)
            self.norm2 = ME.MinkowskiBatchNorm(planes, momentum=bn_momentum)
            self.relu = ME.MinkowskiReLU(inplace=True)
            self.downsample = downsample

        def forward(self, x):
            residual = x
            out = self.conv1(x)
            if _ibn is not None:
                out = _ibn(self.bn_norm1, self.in_norm1, out)
            else:
                out = self.relu(ME.cat(self.bn_norm1(out), self.in_norm1(out)))
            if _conv_bn is not None:   # norm2 + residual + ReLU as one fused pass behind conv2 (as in BasicBlock)
                if self.downsample is not None:
                    residual = self.downsample(x)
                return _conv_bn(self.conv2, self.norm2, out, relu=True, residual=residual)
            out = self.norm2(self.conv2(out))
            if self.downsample is not None:
                residual = self.downsample(x)
            out += residual
            return self.relu(out)

    class RobustBlock(nn.Module):
        """minkunet_robustnet.py:9-53: conv1 -> norm1 (BN) -> ReLU -> conv2 -> norm2 -> += downsample(x) or x ->
        in_norm1 (InstanceNorm); no ReLU at the end of the block (the caller applies one, in place)"""
        expansion = 1

        def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, bn_momentum=0.1, dimension=-1):
            super().__init__()
            assert dimension > 0
            self.conv1 = ME.MinkowskiConvolution(inplanes, planes, kernel_size=3, stride=stride, dilation=dilation,
                                                 dimension=dimension)
            self.in_norm1 = ME.MinkowskiInstanceNorm(planes)
            self.norm1 = ME.MinkowskiBatchNorm(planes, momentum=bn_momentum)
            self.conv2 = ME.MinkowskiConvolution(planes, planes, kernel_size=3, stride=1, dilation=dilation,
                                                 dimension=dimension)
            self.norm2 = ME.MinkowskiBatchNorm(planes, momentum=bn_momentum)
            self.relu = ME.MinkowskiReLU(inplace=True)
            self.downsample = downsample

        def forward(self, x):
            residual = x if self.downsample is None else None
            if _conv_bn is not None:   # BN statistics from the convolutions' epilogues; norm2 + residual in one pass
                out = _conv_bn(self.conv1, self.norm1, x, relu=True)
                if self.downsample is not None:
                    residual = self.downsample(x)
                out = _conv_bn(self.conv2, self.norm2, out, relu=False, residual=residual)
            else:
                out = self.relu(self.norm1(self.conv1(x)))
                out = self.norm2(self.conv2(out))
                if self.downsample is not None:
                    residual = self.downsample(x)
                out += residual
            return self.in_norm1(out)

    class _Trunk(nn.Module):
        BLOCK = BasicBlock
        LAYERS = LAYERS34
        EXECUTOR = True     # the training-mode trunk may go to the executor (it knows BasicBlocks only)

        def _stage_block(self, stage):
            return self.BLOCK

        def _build_trunk(self, in_channels, out_channels, D, initial_kernel_size):
            self.D = D
            self.inplanes = INIT_DIM
            self.conv0p1s1 = ME.MinkowskiConvolution(in_channels, INIT_DIM, kernel_size=initial_kernel_size,
                                                     dimension=D)
            self.bn0 = ME.MinkowskiBatchNorm(INIT_DIM)
            for i, s in _ENC:
                setattr(self, f"conv{i}p{s}s2", ME.MinkowskiConvolution(self.inplanes, self.inplanes, kernel_size=2,
                                                                       stride=2, dimension=D))
                setattr(self, f"bn{i}", ME.MinkowskiBatchNorm(self.inplanes))
                setattr(self, f"block{i}", self._make_layer(PLANES[i - 1], self.LAYERS[i - 1], self._stage_block(i)))
            skips = [PLANES[2], PLANES[1], PLANES[0], INIT_DIM]
            for (j, s), skip in zip(_DEC, skips):
                setattr(self, f"convtr{j}p{s}s2", ME.MinkowskiConvolutionTranspose(self.inplanes, PLANES[j],
                                                                                  kernel_size=2, stride=2,
                                                                                  dimension=D))
                setattr(self, f"bntr{j}", ME.MinkowskiBatchNorm(PLANES[j]))
                self.inplanes = PLANES[j] + skip
                setattr(self, f"block{j + 1}", self._make_layer(PLANES[j], self.LAYERS[j], self._stage_block(j + 1)))
            self.final = ME.MinkowskiConvolution(PLANES[7], out_channels, kernel_size=1, bias=True, dimension=D)
            self.relu = ME.MinkowskiReLU(inplace=True)
            self.dropout = ME.MinkowskiDropout(p=0.5)  # constructed, never called (minkunet_bev.py:126)

        def _build_mixstyle(self, layers, p, alpha, seed):
            """MixStyle (ME.MinkowskiMixStyle, include/lidog_amd.h) behind the named encoder stages: weightless modules,
            registered last and only when asked for, so state_dict keys and their order never change.  Every module
            draws from its own RandomState, seeded with (seed, stage number)."""
            layers = tuple(layers)
            stages = [f"block{i}" for i, _ in _ENC]
            if any(name not in stages for name in layers) or len(set(layers)) != len(layers):
                raise ValueError(f"mixstyle_layers {list(layers)}: distinct stages among {', '.join(stages)}")
            if layers:
                self.mixstyle = nn.ModuleDict({name: ME.MinkowskiMixStyle(p=p, alpha=alpha, seed=[seed, int(name[5:])])
                                               for name in sorted(layers)})

        def _mixstyle_training(self):
            """MixStyle may act in this forward pass: the operator path runs it (the executor knows BasicBlocks only)"""
            return self.training and "mixstyle" in self._modules

        def _mix(self, stage, x):
            mods = self._modules.get("mixstyle")
            return mods[stage](x) if mods is not None and stage in mods else x

        def _make_layer(self, planes, blocks, block):
            downsample = None
            if self.inplanes != planes:
                downsample = nn.Sequential(
                    ME.MinkowskiConvolution(self.inplanes, planes, kernel_size=1, stride=1, dimension=self.D),
                    ME.MinkowskiBatchNorm(planes))
            layers = [block(self.inplanes, planes, stride=1, dilation=1, downsample=downsample, dimension=self.D)]
            self.inplanes = planes
            for _ in range(1, blocks):
                layers.append(block(self.inplanes, planes, stride=1, dilation=1, dimension=self.D))
            return nn.Sequential(*layers)

        def weight_initialization(self):
            # minkunet_bev.py:401-408: only MinkowskiConvolution (not ...Transpose) gets kaiming fan_out
            for m in self.modules():
                if isinstance(m, ME.MinkowskiConvolution):
                    ME.utils.kaiming_normal_(m.kernel, mode="fan_out", nonlinearity="relu")
                if isinstance(m, ME.MinkowskiBatchNorm):
                    nn.init.constant_(m.bn.weight, 1)
                    nn.init.constant_(m.bn.bias, 0)

        def _bn_relu(self, bn, x):
            return _fused(bn, x) if _fused is not None else self.relu(bn(x))

        def _conv_bn_relu(self, conv, bn, x):
            if _conv_bn is not None:  # backend fast path: BN statistics from the convolution's own epilogue
                return _conv_bn(conv, bn, x, relu=True)
            return self._bn_relu(bn, conv(x))

        def _trunk_forward(self, x):
            """returns (out_block8, out_bottle, {level: tensor}, classifier output or None = not computed yet)"""
            if _trunk_exec is not None and self.EXECUTOR and not self._mixstyle_training():
                done = _trunk_exec(self, x)
                if done is not None:
                    return done
            out = self._conv_bn_relu(self.conv0p1s1, self.bn0, x)
            skips = [out]
            for i, s in _ENC:
                out = self._conv_bn_relu(getattr(self, f"conv{i}p{s}s2"), getattr(self, f"bn{i}"), out)
                out = self._mix(f"block{i}", getattr(self, f"block{i}")(out))
                skips.append(out)
            bottle = skips.pop()
            levels = {}
            names = ["bottle", "block6", "block7", "block8"]
            for (j, s), name in zip(_DEC, names):
                out = self._conv_bn_relu(getattr(self, f"convtr{j}p{s}s2"), getattr(self, f"bntr{j}"), out)
                out = ME.cat(out, skips.pop())
                out = getattr(self, f"block{j + 1}")(out)
                levels[name] = out
            return out, bottle, levels, None

    class MinkUNet34(_Trunk):
        def __init__(self, in_channels, out_channels, D=3, initial_kernel_size=5, mixstyle_layers=(), mixstyle_p=0.5,
                     mixstyle_alpha=0.1, mixstyle_seed=0):
            super().__init__()
            self._build_trunk(in_channels, out_channels, D, initial_kernel_size)
            self.weight_initialization()
            self._build_mixstyle(mixstyle_layers, mixstyle_p, mixstyle_alpha, mixstyle_seed)

        def forward(self, x, is_seg=True):
            out, _, _, seg = self._trunk_forward(x)
            seg = seg if seg is not None else self.final(out)
            return seg if is_seg else (seg, out)

    class MinkUNet34BEV(_Trunk):
        def __init__(self, in_channels, out_channels, D, initial_kernel_size=5, dynamic_mapping=False,
                     decoder_2d_level=("block8",), bottle_img_dim=None, bottle_out_img_dim=None,
                     mapping_bound_2d=50.0, scaling_factors=None, binary_seg_layer=False, mixstyle_layers=(),
                     mixstyle_p=0.5, mixstyle_alpha=0.1, mixstyle_seed=0):
            super().__init__()
            assert not binary_seg_layer, "binary_seg_layer is off in every LiDOG config"
            self.mapping_bound_2d = mapping_bound_2d
            self.decoder_2d_level = list(decoder_2d_level)
            self.scaling_factors = scaling_factors or {k: 1.0 for k in BEV_LEVEL_CHANNELS}
            self._build_trunk(in_channels, out_channels, D, initial_kernel_size)
            self.encoders2d = nn.ModuleDict({k: Encoder2D(BEV_LEVEL_CHANNELS[k], n_classes=out_channels)
                                             for k in self.decoder_2d_level})
            self.weight_initialization()
            self._build_mixstyle(mixstyle_layers, mixstyle_p, mixstyle_alpha, mixstyle_seed)

        def forward(self, x, is_seg=True, is_train=False):
            out, bottle, levels, seg = self._trunk_forward(x)
            img_pred = None
            if is_train:
                img_pred = {}
                for key in self.encoders2d.keys():
                    stride = int(3 / self.scaling_factors[key])
                    bev = sparse2super(levels[key], bound=self.mapping_bound_2d, voxel=0.05, pool=(5, stride, 1))
                    img_pred[key] = self.encoders2d[key](bev)
            seg = seg if seg is not None else self.final(out)
            if is_seg:
                return seg, img_pred
            return seg, img_pred, bottle, None

    class MinkUNet34IBN(_Trunk):
        """IBN-Net baseline (minkunet_ibn.py:209-211): IBN blocks in block1-3, BasicBlocks in block4-8.  The operator
        path runs it (the trunk executor knows BasicBlocks only).  ResNetBase.__init__ drops initial_kernel_size, so
        conv0p1s1 is always 5^3 (resnet_old.py via minkunet_ibn.py:68-69)."""
        EXECUTOR = False

        def __init__(self, in_channels, out_channels, D=3, initial_kernel_size=5, mixstyle_layers=(), mixstyle_p=0.5,
                     mixstyle_alpha=0.1, mixstyle_seed=0):
            super().__init__()
            self._build_trunk(in_channels, out_channels, D, 5)
            self.weight_initialization()
            self._build_mixstyle(mixstyle_layers, mixstyle_p, mixstyle_alpha, mixstyle_seed)

        def _stage_block(self, stage):
            return IBNBlock if stage <= 3 else BasicBlock

        def forward(self, x, is_seg=True):
            out, bottle, _, _ = self._trunk_forward(x)
            seg = self.final(out)
            return seg if is_seg else (seg, bottle)

    class MinkUNet34Robust(_Trunk):
        """RobustNet baseline (minkunet_robustnet.py:227-230): instance norms in0 / in1 after conv0p1s1 / conv1p1s2,
        RobustBlocks in block1-3, BasicBlocks in block4-8, the MinkUNet34 decoder.  The operator path runs it (the trunk
        executor knows BasicBlocks only).  ResNetBase.__init__ drops initial_kernel_size, so conv0p1s1 is always 5^3.

        forward(x, is_seg=False) returns (logits, (out_in0, out_in1, out_in1p2, out_in2p4, out_in3p8)), the maps of the
        instance-whitening loss.  The reference passes out_in0 and the three block outputs to MinkowskiReLU(inplace=True)
        afterwards, so the tuple holds them ReLU'd; its second ReLU acts on conv1p1s2's output, not on out_in1, which
        therefore stays un-ReLU'd (the [ME-mem] convention next to lidog_amd.me.IN_EPS)."""
        EXECUTOR = False

        def __init__(self, in_channels, out_channels, D=3, initial_kernel_size=5, mixstyle_layers=(), mixstyle_p=0.5,
                     mixstyle_alpha=0.1, mixstyle_seed=0):
            super().__init__()
            self.D = D
            # minkunet_robustnet.py:68-158, in registration order (state_dict keys)
            self.inplanes = INIT_DIM
            self.conv0p1s1 = ME.MinkowskiConvolution(in_channels, INIT_DIM, kernel_size=5, dimension=D)
            self.in0 = ME.MinkowskiInstanceNorm(INIT_DIM)
            self.conv1p1s2 = ME.MinkowskiConvolution(INIT_DIM, INIT_DIM, kernel_size=2, stride=2, dimension=D)
            self.in1 = ME.MinkowskiInstanceNorm(INIT_DIM)
            self.block1 = self._make_layer(PLANES[0], self.LAYERS[0], RobustBlock)
            for i, s in _ENC[1:]:
                setattr(self, f"conv{i}p{s}s2", ME.MinkowskiConvolution(self.inplanes, self.inplanes, kernel_size=2,
                                                                       stride=2, dimension=D))
                setattr(self, f"bn{i}", ME.MinkowskiBatchNorm(self.inplanes))
                setattr(self, f"block{i}", self._make_layer(PLANES[i - 1], self.LAYERS[i - 1],
                                                            RobustBlock if i <= 3 else BasicBlock))
            skips = [PLANES[2], PLANES[1], PLANES[0], INIT_DIM]
            for (j, s), skip in zip(_DEC, skips):
                setattr(self, f"convtr{j}p{s}s2", ME.MinkowskiConvolutionTranspose(self.inplanes, PLANES[j],
                                                                                  kernel_size=2, stride=2,
                                                                                  dimension=D))
                setattr(self, f"bntr{j}", ME.MinkowskiBatchNorm(PLANES[j]))
                self.inplanes = PLANES[j] + skip
                setattr(self, f"block{j + 1}", self._make_layer(PLANES[j], self.LAYERS[j], BasicBlock))
            self.final = ME.MinkowskiConvolution(PLANES[7], out_channels, kernel_size=1, bias=True, dimension=D)
            self.relu = ME.MinkowskiReLU(inplace=True)
            self.dropout = ME.MinkowskiDropout(p=0.5)  # constructed, never called
            self.weight_initialization()
            self._build_mixstyle(mixstyle_layers, mixstyle_p, mixstyle_alpha, mixstyle_seed)

        def forward(self, x, is_seg=True):
            # minkunet_robustnet.py:160-224
            out = self.conv0p1s1(x)
            out_in0 = self.in0(out)
            out_p1 = self.relu(out_in0)            # in place: out_in0 holds the ReLU'd features from here on
            out = self.conv1p1s2(out_p1)
            out_in1 = self.in1(out)
            # the reference's in-place ReLU of conv1p1s2's output: out of place here, because in1 keeps that output
            # for its backward pass (same values; out_in1 is not ReLU'd either way)
            out = ME.MinkowskiReLU()(out)
            out_in1p2 = self.block1(out)
            # MixStyle acts on what the next stage and the skip read; the maps of the whitening loss stay as they are
            out_b1p2 = self._mix("block1", self.relu(out_in1p2))
            out = self._conv_bn_relu(self.conv2p2s2, self.bn2, out_b1p2)
            out_in2p4 = self.block2(out)
            out_b2p4 = self._mix("block2", self.relu(out_in2p4))
            out = self._conv_bn_relu(self.conv3p4s2, self.bn3, out_b2p4)
            out_in3p8 = self.block3(out)
            out_b3p8 = self._mix("block3", self.relu(out_in3p8))
            out = self._conv_bn_relu(self.conv4p8s2, self.bn4, out_b3p8)
            out = self._mix("block4", self.block4(out))
            skips = [out_p1, out_b1p2, out_b2p4, out_b3p8]
            for j, s in _DEC:
                out = self._conv_bn_relu(getattr(self, f"convtr{j}p{s}s2"), getattr(self, f"bntr{j}"), out)
                out = ME.cat(out, skips.pop())
                out = getattr(self, f"block{j + 1}")(out)
            seg = self.final(out)
            if is_seg:
                return seg
            return seg, (out_in0, out_in1, out_in1p2, out_in2p4, out_in3p8)

    return types.SimpleNamespace(MinkUNet34=MinkUNet34, MinkUNet34BEV=MinkUNet34BEV, MinkUNet34IBN=MinkUNet34IBN,
                                 IBNBlock=IBNBlock, MinkUNet34Robust=MinkUNet34Robust, RobustBlock=RobustBlock)
