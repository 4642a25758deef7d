"""Segmentors on the HIP kernels -- registry keys `EncoderDecoder`, `EventsEncoderDecoder`, `FusionEncoderDecoder`.

Mirrors mmseg/models/segmentors/encoder_decoder.py (EncoderDecoder :19-300; FusionEncoderDecoder :625-1003:
extract_feat :698-721, encode_decode :723-746, forward_train :794-831) and base.py `_parse_losses` :710-743.
The whole student pass (backbones -> fusion -> decode head -> fused up-sample + CE) is scheduled by hand on the
kernel library; autograd sees one node per forward_train (`_TrainFn`) whose backward replays the hand-written
backward pass and accumulates parameter gradients in place.
"""
from collections import OrderedDict

import os

import torch
import torch.nn as nn

from . import deferred, ops
from . import runtime as rt
from .registry import SEGMENTORS, build_backbone, build_fusion, build_head


def add_prefix(d, prefix):
    return {f'{prefix}.{k}': v for k, v in d.items()}


def parse_losses(losses):
    """base.py:710-743 without the host syncs: returns (loss tensor, log_vars of *device* scalars)."""
    log_vars = OrderedDict()
    for name, value in losses.items():
        if isinstance(value, torch.Tensor):
            log_vars[name] = value.mean()
        elif isinstance(value, list):
            log_vars[name] = sum(v.mean() for v in value)
        else:
            raise TypeError(f'{name} is not a tensor or list of tensors')
    loss = sum(v for k, v in log_vars.items() if 'loss' in k)
    log_vars['loss'] = loss
    return loss, log_vars


def _first_meta(img_metas):
    """the (first) image's meta dict; {} when there is none"""
    return (img_metas[0] if isinstance(img_metas, (list, tuple)) else img_metas) or {}


def _resize_logits(seg_logit, ori_shape):
    """NCHW logits at the size ori_shape[:2] (the test pipeline's `rescale`)"""
    h, w = ori_shape[:2]
    if (h, w) != tuple(seg_logit.shape[2:]):
        seg_logit = ops.upsample_logits_nchw(seg_logit.permute(0, 2, 3, 1).contiguous(), h, w)
    return seg_logit


def _flip_back(seg, meta):
    """undo the test pipeline's flip"""
    if meta.get('flip'):
        assert meta['flip_direction'] in ('horizontal', 'vertical')
        seg = seg.flip(dims=(3,) if meta['flip_direction'] == 'horizontal' else (2,))
    return seg


def _label_maps(seg):
    """per-image label maps (numpy) from NCHW logits or probabilities"""
    return list(seg.argmax(dim=1).cpu().numpy())


_FLIP_CODES = {'horizontal': ops.FLIP_HORIZONTAL, 'vertical': ops.FLIP_VERTICAL}


def _slide_cfg(model):
    """None under test_cfg.mode 'whole'; (crop_size, stride) under test_cfg = dict(mode='slide', crop_size=(h, w), stride=(h, w))"""
    cfg = model.test_cfg or {}
    mode = cfg.get('mode', 'whole')
    if mode == 'whole':
        return None
    if mode != 'slide':
        raise NotImplementedError(f"{type(model).__name__}: test_cfg.mode '{mode}' (only 'whole' and 'slide' are implemented)")
    crop, stride = cfg.get('crop_size'), cfg.get('stride')
    if crop is None or stride is None:
        raise NotImplementedError(f"{type(model).__name__}: test_cfg.mode 'slide' needs crop_size=(h, w) and stride=(h, w)")
    return (int(crop[0]), int(crop[1])), (int(stride[0]), int(stride[1]))


def _flip_code(meta):
    if not meta.get('flip'):
        return ops.FLIP_NONE
    assert meta['flip_direction'] in _FLIP_CODES
    return _FLIP_CODES[meta['flip_direction']]


def _window_logits(model, spatial, run, crop, stride):
    """Low-resolution logits of every window of the grid, fp32 NHWC [K,B,hl,wl,nc] (window order of `ops.slide_windows`).  Every
    spatial input of the sample (`spatial`: name -> NCHW tensor, all of one size) is cropped with the same window and the windows
    go through the network (`run(spatial) -> fp32 NHWC logits`) as ONE batch of K*B samples, window-major, where the reference
    loops over them (encoder_decoder.py:190-204).  `model.slide_batch` caps the windows per pass (None: all; 1: the reference's
    loop)."""
    B, _, H, W = next(iter(spatial.values())).shape
    wins = ops.slide_windows(H, W, crop, stride)
    per = getattr(model, 'slide_batch', None) or len(wins)
    parts = []
    for first in range(0, len(wins), per):
        chunk = wins[first:first + per]
        batch = {k: torch.cat([t[:, :, y1:y2, x1:x2] for y1, x1, y2, x2 in chunk]).contiguous() for k, t in spatial.items()}
        logits = run(batch)
        parts.append(logits.reshape((len(chunk), B) + tuple(logits.shape[1:])))
    return wins, (parts[0] if len(parts) == 1 else torch.cat(parts))


def _slide_inference(model, spatial, run, meta, rescale):
    """the reference's slide_inference (encoder_decoder.py:175-218) restated with full-size tensors, the path `inference` and
    `simple_test` take: NCHW logits = (sum over the windows, in order, of the window's logits up-sampled to the window and
    zero-padded to the image) / (the number of windows per pixel), resized to meta['ori_shape'] when `rescale`"""
    crop, stride = _slide_cfg(model)
    wins, logits = _window_logits(model, spatial, run, crop, stride)
    _, B, _, _, nc = logits.shape
    H, W = next(iter(spatial.values())).shape[2:]
    preds = torch.zeros(B, nc, H, W, dtype=torch.float32, device=logits.device)
    count = torch.zeros(B, 1, H, W, dtype=torch.float32, device=logits.device)
    for k, (y1, x1, y2, x2) in enumerate(wins):
        preds += nn.functional.pad(ops.upsample_logits_nchw(logits[k], y2 - y1, x2 - x1), (x1, W - x2, y1, H - y2))
        count[:, :, y1:y2, x1:x2] += 1
    preds = preds / count
    if rescale and meta.get('ori_shape') is not None:
        preds = _resize_logits(preds, meta['ori_shape'])
    return preds


def _view_logits(model, spatial, run):
    """one view's window logits [K,B,hl,wl,nc] with their grid (H, W, crop, stride); 'whole' is the grid of one window"""
    H, W = next(iter(spatial.values())).shape[2:]
    slide = _slide_cfg(model)
    if slide is None:
        return run(spatial)[None], H, W, (H, W), (H, W)
    return _window_logits(model, spatial, run, *slide)[1], H, W, slide[0], slide[1]


def _predict_labels(model, spatial, run, meta, rescale, gt_semantic_seg, meter):
    """shared tail of every segmentor's `predict`: uint8 device label maps [B,OH,OW] in ONE launch behind the network.
    'whole': `ops.seg_predict` on the low-resolution fp32 NHWC logits `run(spatial)` (up-sample to the input size, resize to the
    meta's `ori_shape` when `rescale`, flip back, arg-max -- what `simple_test` computes through full-size logits and a host copy).
    'slide': the windows as one batch (`_window_logits`), then `ops.seg_predict_windows` (window sum, divide, resize, flip back,
    arg-max; no nc x H x W tensor per window or per image).  With `meter` (metrics.ConfusionMeter) and `gt_semantic_seg` the same
    launch adds the image's confusion counters to the meter."""
    slide = _slide_cfg(model)
    out_hw = tuple(meta['ori_shape'][:2]) if rescale and meta.get('ori_shape') is not None else None
    flip = _flip_code(meta)
    H, W = next(iter(spatial.values())).shape[2:]
    score = () if meter is None or gt_semantic_seg is None else (meter._label_tensor(gt_semantic_seg), meter.conf, meter.ignore_index)
    if slide is None:
        return ops.seg_predict(run(spatial), H, W, out_hw, flip, *score)
    logits = _window_logits(model, spatial, run, *slide)[1]
    return ops.seg_predict_windows(logits, H, W, slide[0], slide[1], out_hw, flip, *score)


def _predict_aug(model, views, gt_semantic_seg, meter):
    """shared body of every segmentor's `predict_aug`: `aug_test` without leaving the device.  views: [(spatial, run, meta)].  One
    `ops.seg_prob_accumulate` launch per view (the view's soft-max at `ori_shape`, flipped back, written to / added into ONE fp32
    [B,nc,OH,OW] accumulator; whole or slide mode), then one `ops.prob_predict` launch (divide by the number of views, arg-max,
    and the confusion counters when `meter` and `gt_semantic_seg` are given)."""
    assert len(views) >= 1
    out_hw = tuple(views[0][2]['ori_shape'][:2])
    acc = None
    for i, (spatial, run, meta) in enumerate(views):
        assert tuple(meta['ori_shape'][:2]) == out_hw, 'the views of one image share its ori_shape'
        logits, H, W, crop, stride = _view_logits(model, spatial, run)
        if acc is None:
            acc = torch.empty((logits.shape[1], logits.shape[4]) + out_hw, dtype=torch.float32, device=logits.device)
        ops.seg_prob_accumulate(logits, H, W, crop, stride, out_hw, _flip_code(meta), acc, i > 0)
    if meter is None or gt_semantic_seg is None:
        return ops.prob_predict(acc, len(views))
    return ops.prob_predict(acc, len(views), meter._label_tensor(gt_semantic_seg), meter.conf, meter.ignore_index)


def _aug_labels(probs):
    """the end of the reference's aug_test (encoder_decoder.py:295-304): the views' probabilities summed in order, divided by their
    number, arg-max; per-image label maps (numpy)"""
    seg = probs[0]
    for p in probs[1:]:
        seg += p
    seg /= len(probs)
    return _label_maps(seg)


class _TrainFn(torch.autograd.Function):
    """loss = runner.train_fwd(...); backward(dloss) -> runner.train_bwd(saved, dloss).  A pass with a feature-consistency term
    (FusionEncoderDecoder, `no_fusion` route) returns (loss_seg, loss_feat_consis) and back-propagates each with its own incoming
    gradient."""

    @staticmethod
    def forward(ctx, runner, anchor, args):
        loss, aux, saved = runner.train_fwd(*args)
        ctx.runner, ctx.saved = runner, saved
        ctx.aux = aux
        extra = aux[0].get('loss_feat_consis') if isinstance(aux[0], dict) else None
        ctx.two = extra is not None
        return (loss, extra.view(())) if ctx.two else loss

    @staticmethod
    def backward(ctx, dloss, dextra=None):
        g = dloss.contiguous().float().view(1)
        if ctx.two:
            ctx.runner.train_bwd(ctx.saved, g, fc_gscale=dextra.contiguous().float().view(1))
        else:
            ctx.runner.train_bwd(ctx.saved, g)
        ctx.saved = None
        return None, None, None


@SEGMENTORS.register_module()
class EncoderDecoder(nn.Module):
    """Single-modality MiT + DAFormerHead (BASELINE.json configs[0]/[1])."""

    def __init__(self, backbone, decode_head, neck=None, auxiliary_head=None, train_cfg=None, test_cfg=None,
                 pretrained=None, init_cfg=None):
        super().__init__()
        assert neck is None and auxiliary_head is None
        if pretrained is not None:
            assert backbone.get('pretrained') is None, 'both backbone and segmentor set pretrained weight'
            backbone = dict(backbone, pretrained=pretrained)
        self.backbone = build_backbone(backbone)
        self.decode_head = build_head(decode_head)
        self.align_corners = self.decode_head.align_corners
        self.num_classes = self.decode_head.num_classes
        self.train_cfg, self.test_cfg = train_cfg, test_cfg

    def init_weights(self):
        self.backbone.init_weights()
        self.decode_head.init_weights()

    def extract_feat(self, img):
        return self.backbone(img)

    # hand-scheduled training pass
    def train_fwd(self, img, gt, seg_weight):
        """returns (loss, (losses, logits, feats), saved); feats = the backbone's [(rows [B*N, C], h, w)] * 4"""
        B = img.shape[0]
        feats, sv_b = self.backbone.fwd(img)
        losses, logits, sv_h = self.decode_head.fwd_train(feats, B, gt, seg_weight)
        return losses['loss_seg'], (losses, logits, feats), (sv_b, sv_h, B)

    def train_bwd(self, saved, gscale, img_grad_hook=None):
        """img_grad_hook(d): called with the backbone's four output gradients before its backward pass starts; it may add into
        them in place, or fill a None entry (uda.DACS: the ImageNet feature distance on stage 4)"""
        sv_b, sv_h, B = saved
        with ops.backward_scope():   # LayerNorm parameter gradients of the whole pass folded by one launch at the end
            dfs = self.decode_head.bwd_train(sv_h, B, gscale)
            rt.notify_grads_ready('decode_head', self.decode_head)
            d = [dfs.get(i) for i in range(4)]
            if img_grad_hook is not None:
                img_grad_hook(d)
            self.backbone.bwd(sv_b, d)
        rt.join_lanes('wgrad')

    def forward_train(self, img, img_metas=None, gt_semantic_seg=None, seg_weight=None, return_feat=False):
        holder = {}
        loss = _TrainFn.apply(_Capture(self, holder), rt.anchor(img.device), (img, gt_semantic_seg, seg_weight))
        losses, logits, _ = holder['aux']
        out = add_prefix({'loss_seg': loss, 'acc_seg': losses['acc_seg']}, 'decode')
        return out, logits.permute(0, 3, 1, 2)

    def encode_decode(self, img, img_metas=None):
        B, _, H, W = img.shape
        with torch.no_grad():
            feats, _ = self.backbone.fwd(img, save=False)
            logits, _ = self.decode_head.fwd(feats, B)
            return ops.upsample_logits_nchw(logits, H, W)

    slide_batch = None   # test_cfg.mode 'slide': windows per network pass (None: all windows of an image as one batch)

    def _test_inputs(self, **kwargs):
        """(spatial inputs to crop per window, run(spatial) -> low-resolution fp32 NHWC logits, the image's meta)"""
        return {'img': kwargs['img']}, (lambda s: self.encode_decode_lowres(s['img'])), _first_meta(kwargs.get('img_meta'))

    def slide_inference(self, img, img_meta=None, rescale=True):
        """encoder_decoder.py:175-218 (test_cfg = dict(mode='slide', crop_size=(h, w), stride=(h, w))): NCHW logits of the image
        from its overlapping windows, averaged where they overlap; at img_meta['ori_shape'] when `rescale`"""
        spatial, run, meta = self._test_inputs(img=img, img_meta=img_meta)
        return _slide_inference(self, spatial, run, meta, rescale)

    def _seg_logit(self, img, img_meta, rescale):
        """slide_inference / whole_inference (:175-237): logits at the input size, resized to img_meta['ori_shape'] when `rescale`"""
        if _slide_cfg(self) is not None:
            return self.slide_inference(img, img_meta, rescale)
        seg_logit = self.encode_decode(img, img_meta)
        meta = _first_meta(img_meta)
        if rescale and meta.get('ori_shape') is not None:
            seg_logit = _resize_logits(seg_logit, meta['ori_shape'])
        return seg_logit

    def inference(self, img, img_meta=None, rescale=True):
        """encoder_decoder.py:239-272: soft-max of the logits (whole or slide), flipped back when the test pipeline flipped"""
        return _flip_back(torch.softmax(self._seg_logit(img, img_meta, rescale), dim=1), _first_meta(img_meta))

    def simple_test(self, img, img_meta=None, rescale=True):
        """encoder_decoder.py:222-285: logits at the input size (test_cfg mode 'whole', or 'slide' from overlapping windows),
        resized to img_meta['ori_shape'] when `rescale`, flipped back when the test pipeline flipped; per-image label maps (numpy)
        -- the reference's soft-max before the argmax is monotone and skipped."""
        return _label_maps(_flip_back(self._seg_logit(img, img_meta, rescale), _first_meta(img_meta)))

    def aug_test(self, imgs, img_metas, rescale=True):
        """encoder_decoder.py:287-304: the views' `inference` outputs (multi-scale / flipped inputs, all rescaled to the image's
        ori_shape) averaged, arg-max; per-image label maps (numpy).  Only rescale=True, as in the reference."""
        assert rescale
        return _aug_labels([self.inference(img, meta, rescale) for img, meta in zip(imgs, img_metas)])

    def encode_decode_lowres(self, img, events=None, test_cfg=None):
        """fp32 NHWC logits [B, H/4, W/4, nc]"""
        with torch.no_grad():
            feats, _ = self.backbone.fwd(img, save=False)
            logits, _ = self.decode_head.fwd(feats, img.shape[0])
        return logits

    def predict(self, rescale=True, gt_semantic_seg=None, meter=None, **kwargs):
        """`simple_test` without leaving the device (keyword inputs `img`, `img_meta`; test_cfg mode 'whole' or 'slide'): uint8
        device label maps [B,OH,OW]"""
        return _predict_labels(self, *self._test_inputs(**kwargs), rescale, gt_semantic_seg, meter)

    def predict_aug(self, samples, gt_semantic_seg=None, meter=None):
        """`aug_test` without leaving the device; samples: one keyword dict per view, as `predict` takes them: uint8 device label
        maps [B,OH,OW] at the views' common ori_shape"""
        return _predict_aug(self, [self._test_inputs(**kw) for kw in samples], gt_semantic_seg, meter)


@SEGMENTORS.register_module()
class EventsEncoderDecoder(EncoderDecoder):
    """encoder_decoder.py:308-620 for the image-only train types 'cs2dsec_image' / 'cs2dz_image' (DAFormer's DACS baseline): one
    MiT on the 3-channel image, a plain DAFormerHead.  The reference also accepts events (concatenated to the image, or alone,
    :365-374); those forms are out of scope here and raise.  State-dict keys: `backbone.*`, `decode_head.*`, as the reference's."""

    def __init__(self, backbone, decode_head, neck=None, auxiliary_head=None, train_cfg=None, test_cfg=None, pretrained=None,
                 init_cfg=None, **kwargs):
        in_chans = backbone.get('in_chans', 3)
        if in_chans != 3:
            raise ValueError(f'EventsEncoderDecoder: in_chans={in_chans}; only the image-only form (in_chans=3, events=None) is '
                             'implemented -- the concatenated image+events and the events-only inputs are not')
        super().__init__(backbone, decode_head, neck, auxiliary_head, train_cfg, test_cfg, pretrained, init_cfg)

    @staticmethod
    def _image_only(image, events):
        if events is not None:
            raise NotImplementedError('EventsEncoderDecoder: event inputs (image+events concatenated, or events alone) are not '
                                      'implemented; pass events=None')
        if image is None:
            raise ValueError('EventsEncoderDecoder: an image is required')
        return image

    def extract_feat(self, image, events=None):
        return self.backbone(self._image_only(image, events))

    def forward_train(self, image, events, gt_semantic_seg, seg_weight=None, return_feat=False):
        """encoder_decoder.py:446-482: (losses, seg_logits) -- seg_logits NCHW fp32 at 1/4 resolution"""
        img = self._image_only(image, events)
        holder = {}
        loss = _TrainFn.apply(_Capture(self, holder), rt.anchor(img.device), (img, gt_semantic_seg, seg_weight))
        losses, logits, feats = holder['aux']
        out = {}
        if return_feat:
            out['features'] = feats
        out.update(add_prefix({'loss_seg': loss, 'acc_seg': losses['acc_seg']}, 'decode'))
        return out, logits.permute(0, 3, 1, 2)

    # -- inference / teacher ---------------------------------------------------------------------------------------------
    def encode_decode_lowres(self, img, events=None, test_cfg=None):
        """fp32 NHWC logits [B, H/4, W/4, nc] (the teacher: the fused pseudo-label kernel up-samples on the fly)"""
        img = self._image_only(img, events)
        with torch.no_grad():
            feats, _ = self.backbone.fwd(img, save=False)
            logits, _ = self.decode_head.fwd(feats, img.shape[0])
        return logits

    def encode_decode(self, img, events=None):
        """:376-387: logits NCHW at the input size"""
        H, W = img.shape[2:]
        return ops.upsample_logits_nchw(self.encode_decode_lowres(img, events), H, W)

    def whole_inference(self, rescale, **kwargs):
        """:525-551: the input keyed by `image`, else `warp_image`; resized to img_metas['ori_shape'] when `rescale`"""
        img = kwargs['image'] if 'image' in kwargs else kwargs.get('warp_image')
        if isinstance(img, list):
            img = img[0]
        events = None if 'image' in kwargs else kwargs.get('events_vg')
        seg_logit = self.encode_decode(img, events)
        if rescale and kwargs.get('img_metas') is not None:
            seg_logit = _resize_logits(seg_logit, _first_meta(kwargs['img_metas'])['ori_shape'])
        return seg_logit

    def _test_inputs(self, **kwargs):
        """(spatial inputs to crop per window, run(spatial) -> low-resolution fp32 NHWC logits, the image's meta); the keyword
        inputs resolved as `whole_inference` does"""
        img = kwargs['image'] if 'image' in kwargs else kwargs.get('warp_image')
        if isinstance(img, list):
            img = img[0]
        events = None if 'image' in kwargs else kwargs.get('events_vg')
        spatial = {'img': img} if events is None else {'img': img, 'events': events}
        return spatial, (lambda s: self.encode_decode_lowres(s['img'], s.get('events'))), _first_meta(kwargs.get('img_metas'))

    def slide_inference(self, rescale, **kwargs):
        """test_cfg = dict(mode='slide', crop_size=(h, w), stride=(h, w)).  The reference's copy of slide_inference in this class
        (:480-520) calls encode_decode with the plain class's signature and cannot run; the behaviour is defined by extension of
        the plain class's (encoder_decoder.py:175-218): every spatial input of the sample (`image` / `warp_image`, `events_vg`)
        is cropped with the same window, everything else as there."""
        spatial, run, meta = self._test_inputs(**kwargs)
        return _slide_inference(self, spatial, run, meta, rescale)

    def inference(self, rescale, **kwargs):
        """:553-588: soft-max of the logits (test_cfg.mode 'whole' or 'slide'), flipped back when the test pipeline flipped"""
        slide = _slide_cfg(self) is not None
        output = torch.softmax(self.slide_inference(rescale, **kwargs) if slide else self.whole_inference(rescale, **kwargs), dim=1)
        return _flip_back(output, _first_meta(kwargs.get('img_metas')))

    def simple_test(self, rescale=True, **kwargs):
        """:590-603: per-image label maps (numpy)"""
        return _label_maps(self.inference(rescale, **kwargs))

    def aug_test(self, samples, rescale=True):
        """Multi-view test; samples: one keyword dict per view, as `simple_test` takes them.  The reference's copy in this class
        (:605-620) calls `inference` with the plain class's signature and cannot run; defined by extension of the plain class's
        (encoder_decoder.py:287-304): the views' `inference` outputs averaged, arg-max; per-image label maps (numpy).  Only
        rescale=True, as in the reference."""
        assert rescale
        return _aug_labels([self.inference(rescale, **kw) for kw in samples])

    def predict(self, rescale=True, gt_semantic_seg=None, meter=None, **kwargs):
        """`simple_test` without leaving the device (the same keyword inputs, resolved as `whole_inference` does; test_cfg mode
        'whole' or 'slide'): uint8 device label maps [B,OH,OW]"""
        return _predict_labels(self, *self._test_inputs(**kwargs), rescale, gt_semantic_seg, meter)


class _Capture:
    """Adapter so that _TrainFn can hand the auxiliary outputs (logits, accuracy) back to forward_train."""

    def __init__(self, model, holder):
        self.model, self.holder = model, holder

    def train_fwd(self, *args):
        loss, aux, saved = self.model.train_fwd(*args)
        self.holder['aux'] = aux
        return loss, aux, saved

    def train_bwd(self, saved, gscale, **kw):
        return self.model.train_bwd(saved, gscale, **kw)


def _sum_grads(a, b):
    """element-wise sum of two per-level gradient lists/dicts (entries may be None)."""
    out = []
    for i in range(4):
        x = a[i] if a is not None else None
        y = b[i] if b is not None else None
        if isinstance(a, dict):
            x = a.get(i)
        if isinstance(b, dict):
            y = b.get(i)
        out.append(y if x is None else (x if y is None else ops.axpby(x, y, 1.0, 1.0)))
    return out


@SEGMENTORS.register_module()
class FusionEncoderDecoder(nn.Module):
    """encoder_decoder.py:625-1003 for train types 'cs2dsec_image+events_together' / 'cs2dsec_image+events' /
    'cs2dz_image+raw-isr' (the ones configs/fusion/* use) and the two-stream 'cs2dz_image+raw-isr_split' (no fusion module: the
    image and the ISR stream each end in their own classifier of the decode head; the teacher pass `encode_decode_lowres(image, isr)`
    returns both outputs, inference reads the events output of `night_isr`, see `_resolve_test_inputs`)."""

    TRAIN_TYPES = {'cs2dsec_image+events', 'cs2dz_image+d2n-isr', 'cs2dz_image+raw-isr', 'cs2dz_image+raw-isr_no-fusion',
                   'cs2dz_image+raw-isr_split', 'cs2dsec_image+events_together'}

    def __init__(self, backbone_image, backbone_events, fusion_module, decode_head, neck=None, auxiliary_head=None,
                 train_cfg=None, test_cfg=None, pretrained=None, init_cfg=None, **kwargs):
        super().__init__()
        assert kwargs['train_type'] in self.TRAIN_TYPES
        self.train_type = kwargs['train_type']
        assert neck is None and auxiliary_head is None
        if pretrained is not None:
            assert backbone_events.get('pretrained') is None and backbone_image.get('pretrained') is None, \
                'both backbone and segmentor set pretrained weight'
            backbone_events = dict(backbone_events, pretrained=pretrained)
            backbone_image = dict(backbone_image, pretrained=pretrained)
        self.backbone_image = build_backbone(backbone_image)
        self.backbone_events = build_backbone(backbone_events)
        if self.train_type in {'cs2dsec_image+events', 'cs2dz_image+raw-isr', 'cs2dsec_image+events_together'}:
            self.fusion_module = build_fusion(fusion_module)
            fim = kwargs.get('fusion_isr_module')
            if fim is not None and fim.get('type', '') != '':
                self.fusion_isr_module = build_fusion(fim)
        else:
            self.fusion_module = None
        self.decode_head = build_head(decode_head)
        self.align_corners = self.decode_head.align_corners
        self.num_classes = self.decode_head.num_classes
        self.train_cfg, self.test_cfg = train_cfg, test_cfg

    def init_weights(self):
        for m in (self.backbone_image, self.backbone_events, self.decode_head):
            m.init_weights()

    # -- feature extraction (extract_feat :698-721) --------------------------------------------------------------
    def _extract(self, image, events, img_self_res, cfg, save):
        cfg = cfg or {}
        B = (image if image is not None else events).shape[0]
        sv = {}
        f_image = f_events = f_isr = None
        if image is not None:
            f_image, sv['image'] = self.backbone_image.fwd(image, save=save)
        if events is not None:
            f_events, sv['events'] = self.backbone_events.fwd(events, save=save)
        if img_self_res is not None:
            f_isr, sv['isr'] = self.backbone_events.fwd(img_self_res, save=save)
        f_fusion = None
        if cfg.get('no_fusion'):
            pass
        elif cfg.get('fusion_isr'):
            second = 'events' if img_self_res is None else 'isr'
            f_fusion, sv['fusion_isr'] = self.fusion_isr_module.fwd(f_image, f_events if second == 'events' else f_isr, B, save)
            sv['fusion_isr_second'] = second
        elif cfg.get('fusion_all'):
            a, sv['fusion_isr'] = self.fusion_isr_module.fwd(f_image, f_isr, B, save)
            sv['fusion_isr_second'] = 'isr'
            b, sv['fusion'] = self.fusion_module.fwd(f_image, f_events, B, save)
            f_fusion = [(ops.axpby(x[0], y[0], 0.5, 0.5), x[1], x[2]) for x, y in zip(a, b)]
            sv['fusion_all'] = True
        elif self.fusion_module is not None and events is not None:
            f_fusion, sv['fusion'] = self.fusion_module.fwd(f_image, f_events, B, save)
        feats = {'f_image': f_image, 'f_events': f_events, 'f_fusion': f_fusion, 'f_img_self_res': f_isr}
        return feats, sv, B

    def _extract_bwd(self, sv, dfeats, B, img_grad_hook=None):
        d_img = dfeats.get('f_image')
        d_evt = dfeats.get('f_events')
        d_isr = dfeats.get('f_img_self_res')
        d_fus = dfeats.get('f_fusion')
        if d_fus is not None:
            d_fus = [d_fus.get(i) for i in range(4)]
            if sv.get('fusion_all'):
                d_fus = [ops.axpby(d, None, 0.5, 0.0) if d is not None else None for d in d_fus]
            if 'fusion' in sv:
                di, de = self.fusion_module.bwd(sv['fusion'], d_fus, B)
                d_img, d_evt = _sum_grads(d_img, di), _sum_grads(d_evt, de)
            if 'fusion_isr' in sv:
                di, de = self.fusion_isr_module.bwd(sv['fusion_isr'], d_fus, B)
                d_img = _sum_grads(d_img, di)
                if sv['fusion_isr_second'] == 'isr':
                    d_isr = _sum_grads(d_isr, de)
                else:
                    d_evt = _sum_grads(d_evt, de)
        as_list = lambda d: [d.get(i) for i in range(4)] if isinstance(d, dict) else d
        if 'image' in sv and d_img is not None:
            d_img = as_list(d_img)
            if img_grad_hook is not None:   # extra terms on the image encoder's output gradients (uda.DACS: ImageNet feature distance)
                img_grad_hook(d_img)
            self.backbone_image.bwd(sv['image'], d_img)
        if 'isr' in sv and d_isr is not None:
            self.backbone_events.bwd(sv['isr'], as_list(d_isr))
        if 'events' in sv and d_evt is not None:
            self.backbone_events.bwd(sv['events'], as_list(d_evt))

    # -- joint pass: events + ISR through the event encoder as ONE batch, all feature sets through the shared decoder at once ----
    def _joint_ok(self, image, events, cfg):
        cfg = cfg or {}
        return (image is not None and events is not None and self.fusion_module is not None
                and not (cfg.get('no_fusion') or cfg.get('fusion_isr') or cfg.get('fusion_all'))
                and hasattr(self.decode_head, 'joint_ok') and self.decode_head.joint_ok()
                and getattr(self, 'joint_passes', True))

    def _extract_joint(self, image, events, img_self_res, save):
        """extract_feat (:698-721) for the default fusion route with the outputs laid out for DAFormerHeadFusion.fwd_joint: per
        level one buffer J_l [G*B*N_l, C_l] holding [image | fusion | events | ISR] blocks.  The image encoder writes block 0,
        the event encoder -- run ONCE over the events and the ISR as a 2B batch (same weights, :703-712) -- blocks 2 and 3, the
        fusion module block 1.  No feature is copied.  Every input may be a LIST of P tensors (the samples of P passes that run
        the same weights, `train_fwd_passes`): B below is then the total over the passes and each block holds pass 0's samples,
        then pass 1's, ..."""
        as_list = lambda t: list(t) if isinstance(t, (list, tuple)) else [t]
        image, events = as_list(image), as_list(events)
        img_self_res = as_list(img_self_res) if img_self_res is not None else None
        B = sum(t.shape[0] for t in image)
        H, W = image[0].shape[2:]
        names = ('image', 'fusion', 'events') + (('isr',) if img_self_res is not None else ())
        G = len(names)
        dims = self.backbone_image.embed_dims
        shapes = self.backbone_image.feature_shapes(H, W)
        dev = image[0].device
        joint = [torch.empty(G * B * h * w, c, dtype=rt.compute_dtype(), device=dev) for (h, w), c in zip(shapes, dims)]
        n = [B * h * w for h, w in shapes]
        ev_in = events + (img_self_res or [])
        with rt.lane('enc', *ev_in, *joint):   # the two encoders are independent until the fusion module: side by side
            f_ev, sv_e = self.backbone_events.fwd(ev_in, save=save, out_feats=[J[2 * m:G * m] for J, m in zip(joint, n)])
        f_image, sv_i = self.backbone_image.fwd(image, save=save, out_feats=[J[:m] for J, m in zip(joint, n)])
        rt.join_lanes('enc')
        f_events = [(J[2 * m:3 * m], h, w) for J, m, (h, w) in zip(joint, n, shapes)]
        # a module with BatchNorm (`per_pass_statistics`) normalises each pass's rows with that pass's statistics and updates its
        # running statistics pass after pass, as the reference's one call per forward does: it is told the number of passes
        per_pass = dict(groups=len(image)) if getattr(self.fusion_module, 'per_pass_statistics', False) else {}
        _, sv_f = self.fusion_module.fwd(f_image, f_events, B, save, into=[J[m:2 * m] for J, m in zip(joint, n)], **per_pass)
        feats = [(J, h, w) for J, (h, w) in zip(joint, shapes)]
        return feats, names, (sv_i, sv_e, sv_f, n, G), B

    def _extract_joint_bwd(self, sv, dJ, B, tail_key=None, img_grad_hook=None):
        """dJ: {level: d J_l}; the gradient blocks are consumed in place (fusion contributions are added into blocks 0 and 2).
        img_grad_hook(d_img): called with the image encoder's four output gradients (rows of every pass, pass 0 first) before its
        backward pass starts -- it may add into them in place"""
        sv_i, sv_e, sv_f, n, G = sv
        d = [dJ.get(i) for i in range(4)]
        d_fus = [(t[m:2 * m] if t is not None else None) for t, m in zip(d, n)]
        di, de = self.fusion_module.bwd(sv_f, d_fus, B)
        ops.gemm_flush_deferred()       # the fusion blocks' queued weight gradients
        d_img, d_ev = [], []
        for t, m, a, b in zip(d, n, di, de):
            if t is None:
                d_img.append(a)
                assert b is None, 'event-encoder gradient without a joint gradient buffer'
                d_ev.append(None)
                continue
            if a is not None:
                ops.axpby(t[:m], a, 1.0, 1.0, out=t[:m])
            if b is not None:
                ops.axpby(t[2 * m:3 * m], b, 1.0, 1.0, out=t[2 * m:3 * m])
            d_img.append(t[:m])
            d_ev.append(t[2 * m:G * m])
        with rt.lane('enc', *[t for t in d if t is not None]):
            self.backbone_events.bwd(sv_e, d_ev)
        if img_grad_hook is not None:
            img_grad_hook(d_img)
        self.backbone_image.bwd(sv_i, d_img)
        if tail_key is not None:   # the decode head's postponed weight gradients: behind the (shorter) image-encoder chain
            ops.run_tail(tail_key)
        rt.join_lanes('enc')
        rt.join_lanes('wgrad')

    # -- hand-scheduled training pass ---------------------------------------------------------------------------------
    def train_fwd(self, inputs, gt, seg_weight, cfg, defer_feat_consis=False):
        """defer_feat_consis: leave the feature-consistency loss (`_feat_consis_on`) to `train_bwd(..., fc_sink=...)`, whose ONE launch
        gives loss and gradient; by default `losses['loss_feat_consis']` is computed here (loss-only launch)"""
        if self._joint_ok(inputs['image'], inputs['events'], cfg):
            feats, names, sv, B = self._extract_joint(inputs['image'], inputs['events'], inputs.get('img_self_res'), True)
            losses, logits, sv_h = self.decode_head.fwd_train_joint(feats, names, B, gt, seg_weight, cfg)
            return losses['loss_seg'], (losses, logits, feats), ('joint', sv, sv_h, B)
        feats, sv, B = self._extract(inputs['image'], inputs['events'], inputs.get('img_self_res'), cfg, True)
        losses, logits, sv_h = self.decode_head.fwd_train(feats, B, gt, seg_weight, cfg)
        if not self._feat_consis_on(cfg):
            return losses['loss_seg'], (losses, logits, feats), (sv, sv_h, B)
        fc = ([f[0] for f in feats['f_image']], [f[0] for f in feats['f_events']], float(cfg['lambda_feature_consistency']))
        if not defer_feat_consis:   # the loss-only launch; train_bwd then runs the gradient-only one
            losses['loss_feat_consis'] = ops.feat_consis(*fc)[0].view(())
        return losses['loss_seg'], (losses, logits, feats), (sv, sv_h, B, fc)

    # -- feature-consistency loss of the `no_fusion` route (forward_train :822-823, :833-848) ------------------------------------
    def _feat_consis_on(self, cfg):
        """train type 'cs2dsec_image+events' with cfg['no_fusion']: lambda * mse_loss(f_image[i], f_events[i].detach()) over the four
        levels joins the loss (f_events: the event encoder's features of the ISR, the second input on these iterations)"""
        return self.train_type == 'cs2dsec_image+events' and bool((cfg or {}).get('no_fusion'))

    @staticmethod
    def _feat_consis_hook(fc, gscale, sink, inner):
        """img_grad_hook: the term's gradient ADDED into the image encoder's four output gradients (the ISR features are detached) --
        one launch; with `sink` the same launch gives the loss (sink(loss [1]), the DACS route), else it is the gradient-only one.
        A level the head left without a gradient gets a zeroed block first.  `inner`: the caller's own hook, run in front."""
        fa, fb, lam = fc

        def hook(d_img):
            if inner is not None:
                inner(d_img)
            given = [d for d in d_img if d is not None]
            for i, a in enumerate(fa):
                if d_img[i] is None:
                    d_img[i] = torch.zeros_like(a, dtype=given[0].dtype if given else a.dtype)
            loss, _ = ops.feat_consis(fa, fb, lam, gscale=gscale, grads=d_img, want_loss=sink is not None)
            if sink is not None:
                sink(loss)
        return hook

    def train_fwd_passes(self, passes, cfg, before_head=None):
        """P training passes with the same weights as ONE pass over P*B samples (passes: list of (inputs, gt, seg_weight)): the
        source and the mixed step of a DACS iteration (dacs.py:489-523, :820-860) differ only in their inputs and targets, and
        the reference's `backward()` calls just add their gradients up.  Per-pass state -- BatchNorm batch statistics and the
        order of the running-statistic updates, the loss normalisation -- is kept per pass (DAFormerHeadFusion.fwd_joint).
        Returns ([(loss, losses)] per pass, saved); `train_bwd(saved, gscale)` back-propagates the SUM of the pass losses.
        before_head: called between the encoders / fusion blocks and the decode head -- the first use of the targets.
        saved[5] = the joint feature buffers [(J_l, h, w)] (block 0 of J_l: the image encoder's rows, pass 0's samples first)."""
        first = passes[0][0]
        assert self._joint_ok(first['image'], first['events'], cfg)
        P = len(passes)
        isr = [p[0]['img_self_res'] for p in passes] if first.get('img_self_res') is not None else None
        feats, names, sv, Bt = self._extract_joint([p[0]['image'] for p in passes], [p[0]['events'] for p in passes], isr, True)
        if before_head is not None:   # the targets (gt, seg_weight) may come from another lane: joined here, behind the encoders (uda.DACS)
            before_head()
        losses, logits, sv_h = self.decode_head.fwd_train_joint(feats, names, Bt // P, [p[1] for p in passes],
                                                                [p[2] for p in passes], cfg, passes=P)
        return [(l['loss_seg'], l) for l in losses], ('joint', sv, sv_h, Bt, P, feats)

    def train_bwd(self, saved, gscale, img_grad_hook=None, fc_gscale=None, fc_sink=None):
        """img_grad_hook: see _extract_joint_bwd (the image encoder's output gradients, before its backward pass).
        fc_gscale: the incoming gradient of the feature-consistency loss (fp32 [1]; None: gscale); fc_sink: see `_feat_consis_hook`"""
        with ops.backward_scope():   # LayerNorm parameter gradients of the whole pass folded by one launch at the end
            if saved[0] == 'joint':
                _, sv, sv_h, B = saved[:4]
                P = saved[4] if len(saved) > 4 else 1
                # TAIL mode (single GPU, lanes on): the decode head's weight gradients (dense GEMMs + the depthwise weight-gradient
                # stencils, ~4 ms at 2 + 2 samples) are off the critical path.  The image encoder's backward chain ends ~2 ms before
                # the event encoder's (half the samples), so they are queued under their own key and launched on the main lane
                # BEHIND the image encoder's backward pass, in the gap before the join.  (With a gradient exchange armed the head's
                # gradients must be final before the encoders start: flushed in place, as before.)
                tail = (rt.concurrency() and rt.grad_ready_hook is None and not rt.lane_enabled('hw') and
                        os.environ.get('CMDA_HEAD_TAIL', '1') != '0')
                with deferred.queue_under('main/headtail' if tail else None):
                    dJ = self.decode_head.bwd_train_joint(sv_h, B // P, gscale)
                if tail:
                    self._extract_joint_bwd(sv, dJ, B, tail_key='main/headtail', img_grad_hook=img_grad_hook)
                    return
                if rt.lane_enabled('hw') and rt.grad_ready_hook is None:
                    # the decode head's queued weight gradients (dense 256 x 256-tile GEMMs, ~3.5 ms at 2 + 2 samples) are off the
                    # critical path: a third queue runs them underneath the encoders' latency-bound backward chains
                    with rt.lane('hw', *deferred.queued_tensors()):
                        ops.gemm_flush_deferred(from_lane='main')
                else:
                    ops.gemm_flush_deferred()   # the decode head's queued weight gradients
                rt.notify_grads_ready('decode_head', self.decode_head)
                self._extract_joint_bwd(sv, dJ, B, img_grad_hook=img_grad_hook)
                rt.join_lanes('hw')
                return
            sv, sv_h, B = saved[:3]
            if len(saved) > 3:   # the feature-consistency term: the same hook point, behind the caller's hook
                img_grad_hook = self._feat_consis_hook(saved[3], gscale if fc_gscale is None else fc_gscale, fc_sink, img_grad_hook)
            dfeats = self.decode_head.bwd_train(sv_h, B, gscale)
            rt.notify_grads_ready('decode_head', self.decode_head)
            self._extract_bwd(sv, dfeats, B, img_grad_hook=img_grad_hook)
            rt.join_lanes('wgrad')

    def forward_train(self, inputs, gt_semantic_seg, seg_weight=None, return_feat=False, cfg=None):
        holder = {}
        dev = inputs['image'].device
        loss = _TrainFn.apply(_Capture(self, holder), rt.anchor(dev), (inputs, gt_semantic_seg, seg_weight, cfg))
        losses, logits, feats = holder['aux']
        out = {}
        if return_feat:
            out['features'] = feats
        if isinstance(loss, tuple):   # (loss_seg, loss_feat_consis): `_feat_consis_on`
            out.update(add_prefix({'loss_seg': loss[0], 'loss_feat_consis': loss[1], 'acc_seg': losses['acc_seg']}, 'decode'))
        else:
            out.update(add_prefix({'loss_seg': loss, 'acc_seg': losses['acc_seg']}, 'decode'))
        pred = {k: (v.permute(0, 3, 1, 2) if v is not None else None) for k, v in logits.items()}
        return out, pred

    # -- inference / teacher ---------------------------------------------------------------------------------------------
    def encode_decode_lowres(self, img, events, img_self_res=None, test_cfg=None):
        """dict of fp32 NHWC logits at 1/4 resolution (the fused kernels up-sample on the fly)."""
        with torch.no_grad():
            if self._joint_ok(img, events, test_cfg):
                feats, names, _, B = self._extract_joint(img, events, img_self_res, False)
                out, _ = self.decode_head.fwd_joint(feats, names, B)
                return out
            feats, _, B = self._extract(img, events, img_self_res, test_cfg, False)
            out, _ = self.decode_head.fwd(feats, B)
        return out

    def encode_decode(self, img, events, img_self_res=None, output_features=False, test_cfg={'output_type': 'fusion'}):
        out = self.encode_decode_lowres(img, events, img_self_res, test_cfg)
        if events is None:
            test_cfg = {'output_type': 'image'}
        H, W = (img if img is not None else events).shape[2:]
        if output_features:
            return {k: (ops.upsample_logits_nchw(v, H, W) if v is not None else None) for k, v in out.items()}
        return ops.upsample_logits_nchw(out[test_cfg['output_type'] + '_output'], H, W)

    def _resolve_test_inputs(self, kwargs):
        """(img, events, test_cfg of encode_decode) from the keyword inputs of the test pipeline (encoder_decoder.py:897-930).
        Split train type (:903-904, :919-920): the events are `night_isr` (required) and the output is the events branch's."""
        img = kwargs['warp_image'] if 'warp_image' in kwargs else kwargs['image']
        test_cfg = kwargs.get('test_cfg') or {'output_type': 'fusion'}
        if self.train_type == 'cs2dz_image+raw-isr_split':
            if kwargs.get('night_isr') is None:
                raise KeyError("night_isr: the train type 'cs2dz_image+raw-isr_split' predicts from the ISR stream; pass night_isr=...")
            return img, kwargs['night_isr'], {'output_type': 'events'}
        if self.train_type in {'cs2dsec_image+events', 'cs2dsec_image+events_together'} and 'events_vg' in kwargs:
            events = kwargs['events_vg']
        elif self.train_type == 'cs2dz_image+raw-isr' and test_cfg['output_type'] == 'image_isr':
            events = kwargs['night_isr']
        else:
            events = None
        if self.train_type == 'cs2dz_image+raw-isr':
            test_cfg = {'output_type': 'fusion'} if test_cfg['output_type'] == 'image_isr' else {'output_type': 'image'}
        return img, events, test_cfg

    def _net_image(self, img):
        """the image the network gets at test time.  Split train type: None -- the reference runs the image stream too and discards its
        output (encode_decode with output_type 'events'); in eval mode that stream has no side effect (BatchNorm reads its running
        statistics, DropPath / Dropout2d are off, nothing joins the two streams), so only the event encoder and the events decoder
        branch run here and the result is exactly the same."""
        return None if self.train_type == 'cs2dz_image+raw-isr_split' else img

    def whole_inference(self, rescale, **kwargs):
        """encoder_decoder.py:897-936: logits at the input size, resized once more to img_metas['ori_shape'] when `rescale`"""
        img, events, test_cfg = self._resolve_test_inputs(kwargs)
        seg_logit = self.encode_decode(self._net_image(img), events, test_cfg=test_cfg)
        if rescale and kwargs.get('img_metas') is not None:
            seg_logit = _resize_logits(seg_logit, _first_meta(kwargs['img_metas'])['ori_shape'])
        return seg_logit

    slide_batch = None   # test_cfg.mode 'slide': windows per network pass (None: all windows of an image as one batch)

    def _test_inputs(self, **kwargs):
        """(spatial inputs to crop per window, run(spatial) -> low-resolution fp32 NHWC logits of the selected output, the meta)"""
        img, events, test_cfg = self._resolve_test_inputs(kwargs)
        key = ('image' if events is None else test_cfg['output_type']) + '_output'   # (encode_decode's rule)
        spatial = {'img': img} if events is None else {'img': img, 'events': events}
        return (spatial, (lambda s: self.encode_decode_lowres(self._net_image(s['img']), s.get('events'), None, test_cfg)[key]),
                _first_meta(kwargs.get('img_metas')))

    def slide_inference(self, rescale, **kwargs):
        """test_cfg = dict(mode='slide', crop_size=(h, w), stride=(h, w)).  The reference's copy of slide_inference in this class
        (:851-894) calls encode_decode with the plain class's signature and cannot run; the behaviour is defined by extension of
        the plain class's (encoder_decoder.py:175-218): every spatial input of the sample (`image` / `warp_image`, `events_vg`,
        `night_isr`) is cropped with the same window, everything else as there."""
        spatial, run, meta = self._test_inputs(**kwargs)
        return _slide_inference(self, spatial, run, meta, rescale)

    def inference(self, rescale, **kwargs):
        """encoder_decoder.py:938-971: soft-max of the logits (test_cfg.mode 'whole' or 'slide'), flipped back when the test
        pipeline flipped"""
        slide = _slide_cfg(self) is not None
        output = torch.softmax(self.slide_inference(rescale, **kwargs) if slide else self.whole_inference(rescale, **kwargs), dim=1)
        return _flip_back(output, _first_meta(kwargs.get('img_metas')))

    def simple_test(self, rescale=True, **kwargs):
        """encoder_decoder.py:973-984: per-image label maps (numpy)"""
        return _label_maps(self.inference(rescale, **kwargs))

    def aug_test(self, samples, rescale=True):
        """Multi-view test; samples: one keyword dict per view, as `simple_test` takes them.  The reference's copy in this class
        (:986-1003) calls `inference` with the plain class's signature and cannot run; defined by extension of the plain class's
        (encoder_decoder.py:287-304): the views' `inference` outputs averaged, arg-max; per-image label maps (numpy).  Only
        rescale=True, as in the reference."""
        assert rescale
        return _aug_labels([self.inference(rescale, **kw) for kw in samples])

    def predict(self, rescale=True, gt_semantic_seg=None, meter=None, **kwargs):
        """`simple_test` without leaving the device (the same keyword inputs; the input / output_type / train_type cases resolved
        as `whole_inference` does; test_cfg mode 'whole' or 'slide'): uint8 device label maps [B,OH,OW]"""
        return _predict_labels(self, *self._test_inputs(**kwargs), rescale, gt_semantic_seg, meter)

    def predict_aug(self, samples, gt_semantic_seg=None, meter=None):
        """`aug_test` without leaving the device; samples: one keyword dict per view: uint8 device label maps [B,OH,OW] at the
        views' common ori_shape"""
        return _predict_aug(self, [self._test_inputs(**kw) for kw in samples], gt_semantic_seg, meter)
