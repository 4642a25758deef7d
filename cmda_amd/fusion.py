"""Image/event feature fusion on the HIP kernels -- registry keys `AttentionAvgFusion`, `AttentionFusion`, `ConvertAvgFusion`,
`AverageFusion` (the reference launcher's `--fusion {attfavg, attf, caf, af}`, my_run_experiments.py:120-140).

Mirrors mmseg/models/fusion/attention_avg_fusion.py:9-51 and attention_fusion.py:9-59 (ctor kwargs, parameter names
`basic_block.{i}.*` / `linear_block.{i}.*`, `forward(image_features, events_features) -> list of 4 maps`).  Features
travel as (NLC tensor [B*H*W, C], H, W) triples; the reference's flatten/transpose/contiguous round trips vanish.
"""
from functools import partial

import torch
import torch.nn as nn

from . import nn as K
from . import ops
from . import runtime as rt
from .backbones import Block, Mlp, draw_drop_path
from .decode_heads import _bn_bwd, _bn_fwd, _bn_stats_ws
from .registry import FUSION

_LN6 = partial(nn.LayerNorm, eps=1e-6)


@FUSION.register_module()
class AttentionAvgFusion(nn.Module):
    def __init__(self, in_channels=[64, 128, 320, 512], num_heads=1, mlp_ratios=4, qkv_bias=True, qk_scale=None,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0.05, norm_layer=_LN6, sr_ratios=[8, 4, 2, 1],
                 act_layer=None, init_cfg=None):
        super().__init__()
        self.basic_block = nn.ModuleList([
            Block(dim=in_channels[i // 2], num_heads=num_heads, mlp_ratio=mlp_ratios, qkv_bias=qkv_bias, qk_scale=qk_scale,
                  drop=drop_rate, attn_drop=attn_drop_rate, drop_path=drop_path_rate, norm_layer=norm_layer,
                  sr_ratio=sr_ratios[i // 2]) for i in range(8)])

    def init_weights(self):
        pass  # the reference keeps torch's default initialisation for these blocks (init_cfg=None)

    @ops.sited('fusion')
    def fwd(self, feats_i, feats_e, B, save=True, into=None):
        """into: optional list of 4 pre-allocated tensors the fused maps are written into.
        The image-side blocks (basic_block[0, 2, 4, 6]) and the event-side blocks (1, 3, 5, 7) never see each other's data before
        the average (attention_avg_fusion.py:45-50): with lanes on, the four event-side blocks run on the side lane next to the four
        image-side ones -- the fusion module was ~4.5 ms of small dependent kernels on ONE lane of the step's single-lane phase."""
        outs, saved = [], []
        draw_drop_path(self, list(self.basic_block), B, feats_i[0][0].device)   # one RNG call for the eight blocks
        pools = [blk._dp_pool[0] for blk in self.basic_block if getattr(blk, '_dp_pool', None) is not None]
        ev = []
        with rt.lane('enc', *[x for x, _, _ in feats_e], *pools):
            for i, (xe, H, W) in enumerate(feats_e):
                ev.append(self.basic_block[2 * i + 1].fwd(xe, B, H, W, save=save))
        im = [self.basic_block[2 * i].fwd(xi, B, H, W, save=save) for i, (xi, H, W) in enumerate(feats_i)]
        rt.join_lanes('enc')
        for i, ((yi, si), (ye, se), (_, H, W)) in enumerate(zip(im, ev, feats_i)):
            self.basic_block[2 * i]._dp_pool = self.basic_block[2 * i + 1]._dp_pool = None
            outs.append((ops.axpby(yi, ye, 0.5, 0.5, out=into[i] if into is not None else None), H, W))
            saved.append((si, se, H, W))
        return outs, saved

    @ops.sited('fusion')
    def bwd(self, saved, dfused, B):
        """dfused: list of 4 gradients (or None).  Returns (d image feats, d event feats) as lists."""
        halves = [ops.axpby(d, None, 0.5, 0.0) if d is not None else None for d in dfused]
        de = [None] * len(saved)
        with rt.lane('enc', *[h for h in halves if h is not None]):
            for i, (si, se, H, W) in enumerate(saved):
                if halves[i] is not None:
                    de[i] = self.basic_block[2 * i + 1].bwd(se, halves[i], B, H, W)
            if rt.concurrency():
                ops.gemm_flush_deferred()   # the side lane's own queue of weight gradients (the caller flushes the current lane's)
        di = [self.basic_block[2 * i].bwd(si, halves[i], B, H, W) if halves[i] is not None else None
              for i, (si, se, H, W) in enumerate(saved)]
        rt.join_lanes('enc')
        return di, de

    def forward(self, image_features, events_features):
        from .decode_heads import _HeadBase
        B = image_features[0].shape[0]
        outs, _ = self.fwd(_HeadBase._to_feats(image_features), _HeadBase._to_feats(events_features), B, save=False)
        return [ops.cast(t, torch.float32).view(B, H, W, -1).permute(0, 3, 1, 2) for t, H, W in outs]


@FUSION.register_module()
class AttentionFusion(nn.Module):
    def __init__(self, in_channels=[64, 128, 320, 512], num_heads=1, mlp_ratios=4, qkv_bias=True, qk_scale=None,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0.05, norm_layer=_LN6, sr_ratios=[8, 4, 2, 1],
                 act_layer=None, init_cfg=None):
        super().__init__()
        self.in_channels = list(in_channels)
        self.basic_block = nn.ModuleList([
            Block(dim=in_channels[i] * 2, num_heads=num_heads, mlp_ratio=mlp_ratios, qkv_bias=qkv_bias, qk_scale=qk_scale,
                  drop=drop_rate, attn_drop=attn_drop_rate, drop_path=drop_path_rate, norm_layer=norm_layer,
                  sr_ratio=sr_ratios[i]) for i in range(4)])
        self.linear_block = nn.ModuleList([
            Mlp(in_features=in_channels[i] * 2, hidden_features=in_channels[i], out_features=in_channels[i])
            for i in range(4)])

    def init_weights(self):
        pass

    @ops.sited('fusion')
    def fwd(self, feats_i, feats_e, B, save=True, into=None):
        outs, saved = [], []
        draw_drop_path(self, list(self.basic_block), B, feats_i[0][0].device)
        for i, ((xi, H, W), (xe, _, _)) in enumerate(zip(feats_i, feats_e)):
            C, M = self.in_channels[i], B * H * W
            cat = torch.empty(M, 2 * C, dtype=rt.compute_dtype(), device=xi.device)
            ops.copy2d(xi, cat, M, C, C, 2 * C)
            ops.copy2d(xe, cat, M, C, C, 2 * C, dst_off=C)
            y, sb = self.basic_block[i].fwd(cat, B, H, W, save=save)
            self.basic_block[i]._dp_pool = None
            z, sm = self.linear_block[i].fwd(y, B, H, W)
            if into is not None:
                z = ops.copy2d(z, into[i], M, C, C, C)
            outs.append((z, H, W))
            saved.append((sb, sm, H, W))
        return outs, saved

    @ops.sited('fusion')
    def bwd(self, saved, dfused, B):
        di, de = [], []
        for i, (sb, sm, H, W) in enumerate(saved):
            d = dfused[i]
            if d is None:
                di.append(None), de.append(None)
                continue
            C, M = self.in_channels[i], B * H * W
            dy = self.linear_block[i].bwd(sm, d, B, H, W)
            dcat = self.basic_block[i].bwd(sb, dy, B, H, W)
            a = torch.empty(M, C, dtype=rt.compute_dtype(), device=d.device)
            b = torch.empty(M, C, dtype=rt.compute_dtype(), device=d.device)
            ops.copy2d(dcat, a, M, C, 2 * C, C)
            ops.copy2d(dcat, b, M, C, 2 * C, C, src_off=C)
            di.append(a), de.append(b)
        return di, de

    def forward(self, image_features, events_features):
        from .decode_heads import _HeadBase
        B = image_features[0].shape[0]
        outs, _ = self.fwd(_HeadBase._to_feats(image_features), _HeadBase._to_feats(events_features), B, save=False)
        return [ops.cast(t, torch.float32).view(B, H, W, -1).permute(0, 3, 1, 2) for t, H, W in outs]


class BasicBlock(nn.Module):
    """Parameter container of the ResNet BasicBlock (backbones/resnet.py:15-100 with its defaults: stride 1, no downsample, BN):
    conv1 / conv2 3x3 without bias, bn1 / bn2 -- the reference's state-dict names."""

    def __init__(self, inplanes, planes):
        super().__init__()
        assert inplanes == planes, 'BasicBlock without a downsample path: the identity add needs inplanes == planes'
        self.planes = planes
        self.conv1 = nn.Conv2d(inplanes, planes, 3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)

    def fwd_head(self, x, B, H, W, groups):
        """conv1 -> bn1 + ReLU -> conv2 -> bn2's statistics; the tail (bn2's apply, + x, ReLU, the average with the sibling block) is
        the module's one ops.resavg_fwd.  Returns the tail's branch and what the backward needs.  Statistics per group of M/groups
        rows; the running statistics take the groups' updates in order (the reference calls the module once per pass)."""
        M, C, dev = B * H * W, self.planes, x.device
        ws = _bn_stats_ws(self.bn1, dev, M, C, groups)
        z1, _, _ = K.conv_fwd(x, self.conv1.weight, None, B, H, W, 1, 1, colstats=None if ws is None else (ws, M // groups))
        y1 = torch.empty(M, C, dtype=rt.compute_dtype(), device=dev)
        st1 = _bn_fwd(self.bn1, z1, y1, M, C, True, groups=groups, stats_ws=ws)
        bn = self.bn2
        ws = _bn_stats_ws(bn, dev, M, C, groups)
        z2, _, _ = K.conv_fwd(y1, self.conv2.weight, None, B, H, W, 1, 1, colstats=None if ws is None else (ws, M // groups))
        if bn.training:
            mean, rstd = ops.bn_stats(z2, bn.running_mean, bn.running_var, M // groups, C, bn.eps, bn.momentum, groups, stats_ws=ws)
        else:
            mean = bn.running_mean.expand(groups, C).contiguous()
            rstd = torch.rsqrt(bn.running_var + bn.eps).expand(groups, C).contiguous()
        return dict(z=z2, x=x, mean=mean, rstd=rstd, gamma=bn.weight, beta=bn.bias), (z1, st1, y1)

    def bwd_head(self, saved, x, dz2, dres, B, H, W, groups):
        """dz2: gradient of conv2's output, dres: the identity path's (both from ops.resavg_bwd); conv1's input gradient is added
        into dres, which is returned"""
        z1, st1, y1 = saved
        M, C = B * H * W, self.planes
        dy1 = K.conv_bwd(dz2, y1, self.conv2.weight, None, B, H, W, 1, 1)
        dz1 = _bn_bwd(self.bn1, dy1, z1, st1, M, C, True, groups=groups)
        return K.conv_bwd(dz1, x, self.conv1.weight, None, B, H, W, 1, 1, dx_out=dres, dx_beta=1.0)


@FUSION.register_module()
class ConvertAvgFusion(nn.Module):
    """convert_avg_fusion.py:8-31: per level one BasicBlock on the image features (basic_block[2l]) and one on the event features
    (basic_block[2l+1]), averaged.  BatchNorm: the module normalises each pass's rows with that pass's statistics
    (`per_pass_statistics`: the joint student pass hands it `groups` = the number of passes laid out one after the other).
    `num_batches_tracked` is not advanced (momentum is fixed: nothing reads it), as in the decode heads."""
    per_pass_statistics = True

    def __init__(self, in_channels=[64, 128, 320, 512], out_channels=[64, 128, 320, 512], init_cfg=None):
        super().__init__()
        self.basic_block = nn.ModuleList([BasicBlock(in_channels[i // 2], out_channels[i // 2]) for i in range(8)])

    def init_weights(self):
        pass  # the reference keeps torch's default initialisation (init_cfg=None)

    @ops.sited('fusion')
    def fwd(self, feats_i, feats_e, B, save=True, into=None, groups=1):
        """groups: the rows of every level are `groups` consecutive blocks (passes) of B/groups samples, each with its own batch
        statistics.  The event-side blocks run on the side lane next to the image-side ones (as in AttentionAvgFusion.fwd), joined in
        front of the tail: ONE ops.resavg_fwd for all levels."""
        assert B % groups == 0
        ev = []
        with rt.lane('enc', *[x for x, _, _ in feats_e]):
            for i, (xe, H, W) in enumerate(feats_e):
                ev.append(self.basic_block[2 * i + 1].fwd_head(xe, B, H, W, groups))
        im = [self.basic_block[2 * i].fwd_head(xi, B, H, W, groups) for i, (xi, H, W) in enumerate(feats_i)]
        rt.join_lanes('enc')
        levels, saved = [], []
        for i, ((bi, si), (be, se), (xi, H, W)) in enumerate(zip(im, ev, feats_i)):
            C = self.basic_block[2 * i].planes
            out = into[i] if into is not None else torch.empty(B * H * W, C, dtype=xi.dtype, device=xi.device)
            levels.append(dict(image=bi, events=be, out=out, M=B * H * W // groups, C=C))
            saved.append((bi, si, be, se, H, W, groups))
        outs = [(o, H, W) for o, (_, H, W) in zip(ops.resavg_fwd(levels, groups), feats_i)]
        return outs, (saved if save else None)

    @ops.sited('fusion')
    def bwd(self, saved, dfused, B):
        """dfused: list of 4 gradients (or None).  Returns (d image feats, d event feats) as lists.  ONE ops.resavg_bwd for all levels,
        then the two convolutions and bn1 of every block, the event side on the side lane."""
        live = [i for i, d in enumerate(dfused) if d is not None]
        di, de = [None] * len(saved), [None] * len(saved)
        if not live:
            return di, de
        levels = []
        for i in live:
            bi, _, be, _, H, W, groups = saved[i]
            blk_i, blk_e = self.basic_block[2 * i], self.basic_block[2 * i + 1]
            levels.append(dict(image=dict(bi, dgamma=rt.grad(blk_i.bn2.weight), dbeta=rt.grad(blk_i.bn2.bias)),
                               events=dict(be, dgamma=rt.grad(blk_e.bn2.weight), dbeta=rt.grad(blk_e.bn2.bias)),
                               dout=dfused[i], M=B * H * W // groups, C=blk_i.planes))
        grads = ops.resavg_bwd(levels, saved[live[0]][6])
        with rt.lane('enc', *[t for _, pair in grads for t in pair]):
            for i, (_, (dz, dres)) in zip(live, grads):
                _, _, be, se, H, W, groups = saved[i]
                de[i] = self.basic_block[2 * i + 1].bwd_head(se, be['x'], dz, dres, B, H, W, groups)
            if rt.concurrency():
                ops.gemm_flush_deferred()   # the side lane's own queue of weight gradients (the caller flushes the current lane's)
        for i, ((dz, dres), _) in zip(live, grads):
            bi, si, _, _, H, W, groups = saved[i]
            di[i] = self.basic_block[2 * i].bwd_head(si, bi['x'], dz, dres, B, H, W, groups)
        rt.join_lanes('enc')
        return di, de

    def forward(self, image_features, events_features):
        from .decode_heads import _HeadBase
        B = image_features[0].shape[0]
        outs, _ = self.fwd(_HeadBase._to_feats(image_features), _HeadBase._to_feats(events_features), B, save=False)
        return [ops.cast(t, torch.float32).view(B, H, W, -1).permute(0, 3, 1, 2) for t, H, W in outs]


@FUSION.register_module()
class AverageFusion(nn.Module):
    """average_fusion.py:5-15: (f_image + f_events) / 2 per level; no parameters."""

    def __init__(self, init_cfg=None):
        super().__init__()

    def init_weights(self):
        pass

    @ops.sited('fusion')
    def fwd(self, feats_i, feats_e, B, save=True, into=None):
        outs = [(ops.axpby(xi, xe, 0.5, 0.5, out=into[i] if into is not None else None), H, W)
                for i, ((xi, H, W), (xe, _, _)) in enumerate(zip(feats_i, feats_e))]
        return outs, ([None] * len(outs) if save else None)

    @ops.sited('fusion')
    def bwd(self, saved, dfused, B):
        """two separately stored halves per level: the joint backward adds into gradient blocks in place"""
        di = [ops.axpby(d, None, 0.5, 0.0) if d is not None else None for d in dfused]
        de = [ops.axpby(d, None, 0.5, 0.0) if d is not None else None for d in dfused]
        return di, de

    def forward(self, image_features, events_features):
        from .decode_heads import _HeadBase
        B = image_features[0].shape[0]
        outs, _ = self.fwd(_HeadBase._to_feats(image_features), _HeadBase._to_feats(events_features), B, save=False)
        return [ops.cast(t, torch.float32).view(B, H, W, -1).permute(0, 3, 1, 2) for t, H, W in outs]
