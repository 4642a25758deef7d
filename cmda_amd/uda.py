"""DACS self-training step of CMDA on the HIP kernels -- registry key `DACS`.

Mirrors mmseg/models/uda/dacs.py::DACS (__init__ :55-242, _init_ema_weights/_update_ema :250-272, train_step :274-315,
forward_train :357-1099) and uda_decorator.py::UDADecoratorFusion :178-252 for the two train types of configs/fusion/*:
'cs2dsec_image+events_together' and 'cs2dz_image+raw-isr' (plus 'cs2dsec_image+events').  What changes is where the
work runs, not what is computed:
  * EMA teacher update: one fused kernel per parameter tensor (or one over the flat buffer when the student's
    parameters live in cmda_amd.optim.FlatAdamW's flat store) instead of a Python loop of torch ops;
  * teacher soft-max / max / threshold count / pseudo-weight: one fused up-sample+argmax kernel on the 1/4-resolution
    logits (no 19 x H x W tensors, no `.cpu()` sync: the confident-pixel count stays on the device);
  * ClassMix of image / events / label / weight: batched kernels (no per-sample Python loop);
  * ISR of the mixed image: on the device (the reference round-trips every sample through PIL on the host);
  * log values stay device scalars (`_parse_losses`' `.item()` syncs are gone); call `log_vars_to_float` when logging.
  * ImageNet feature distance (imnet_feature_dist_lambda > 0, dacs.py:328-354, :566-577): the frozen encoder runs beside the
    teacher, the label rescale / class mask and the masked distance are two kernels (feat_dist.hip), and the distance's gradient is
    added into the student image encoder's stage-4 output gradient of the source rows before that encoder's backward pass.
The image-only train types 'cs2dsec_image' / 'cs2dz_image' (DAFormer's DACS on one MiT and a plain DAFormerHead, the baseline the
fusion types are compared against; dacs.py:363-377 and the image branches below) run through `_iteration_image`: no events, no ISR,
no fusion; for 'cs2dz_image' optionally the frozen 3 -> 3 day -> night generator on the source image (cyclegan_id2in_path).
The split train type 'cs2dz_image+raw-isr_split' (two-stream co-training on Dark Zurich without a fusion block, the ablation row the
fusion result is compared against; dacs.py:611-651, :716-771, :797-802) runs through `_iteration` with the inputs, the mixed image /
ISR and the ISR augmentations of 'cs2dz_image+raw-isr': the teacher's image and events outputs each give their own pseudo-labels,
confident-pixel share and weight map (`ops.split_mix_targets`: both streams' targets in one kernel pair, one class draw shared), and the
mixed step trains each stream on its own targets (dict labels / weights into DAFormerHeadFusion's split loss); the source step passes
the plain label to both streams.  The student runs the two-pass route (no fusion module: no joint pass), on the same lanes.
Refused, with the reason, at construction: 'cs2dz_image+raw-isr_no-fusion' (the reference cannot run it: dacs.py:809 calls
extract_feat(image=None, events=mixed_isr) without cfg and encoder_decoder.py:703 then evaluates cfg.keys() on None),
'cs2dz_image+d2n-isr' (needs pre-translated ISR files that no loader here produces), and the split type together with the ImageNet
feature distance (dacs.py:568-575 ends in an assert for it).
Out of scope here: OrgDACS, LightNet (cyclegan_light_path), the matplotlib debug panels, flare / cow-mask /
deflare augmentations.
ISR augmentations (isr_augment.hip): `sky_mask` (dacs.py:431-434, the source ISR before the student sees it) and `isr_noise_dacs_type`
(dacs.py:753-755, on the ISR recomputed from the mixed image) run as batched launches whose per-sample draws travel in the control
block; the noise fields come from a counter-based generator in the kernel (seed fixed at construction, offset = the iteration counter),
not from torch's generators.
"""
import contextlib
import os
import random
from copy import deepcopy

import numpy as np
import torch
import torch.nn as nn

from . import deferred, ops
from . import runtime as rt
from .cyclegan import define_G
from .parallel import reduce_log_vars
from .registry import UDA, build_segmentor
from .segmentors import add_prefix, parse_losses

_DIRECT = [['leftdown', 'leftup'], ['rightdown', 'rightup']]


def set_stochastic(model, flag):
    """DropPath / Dropout2d on or off without touching BatchNorm's train mode (dacs.py:458-462 for the teacher)."""
    for m in model.modules():
        if hasattr(m, 'drop_path_rate') or hasattr(m, 'dropout_ratio'):
            m.stochastic = flag


def tgt_shape(tgt):
    """shape of the target batch's image tensor (key name differs between the train types)"""
    t = tgt['warp_image'] if 'warp_image' in tgt else tgt['image']
    return t.shape


def log_vars_to_float(log_vars):
    return {k: (v.item() if isinstance(v, torch.Tensor) else v) for k, v in log_vars.items()}


def _freeze(module):
    """no gradients; runtime: the parameters' re-laid-out compute copies survive optimizer steps"""
    for p in module.parameters():
        p.requires_grad_(False)
        p._cmda_frozen = True
    return module


def _frozen_generator(path, **kw):
    """a CycleGAN generator in eval mode, frozen; `path` 'random' = seeded random init (no checkpoint exists offline; bench / tests)"""
    g = define_G(**kw)
    if path != 'random':
        g.load_state_dict(torch.load(path, map_location='cpu'))
    return _freeze(g.eval())


# concurrency lanes of the captured iteration (DACS._capture; CMDA_GRAPH_LANES / DACS.graph_lane_set override): runtime.py documents them
GRAPH_LANES = tuple(x for x in os.environ.get('CMDA_GRAPH_LANES', 'enc,T,Tenc,wq').split(',') if x)


@UDA.register_module()
class DACS(nn.Module):
    SUPPORTED = {'cs2dsec_image+events', 'cs2dz_image+raw-isr', 'cs2dsec_image+events_together', 'cs2dsec_image', 'cs2dz_image',
                 'cs2dz_image+raw-isr_split'}
    SPLIT_TYPE = 'cs2dz_image+raw-isr_split'
    RAW_ISR_TYPES = {'cs2dz_image+raw-isr', 'cs2dz_image+raw-isr_split'}   # Dark Zurich: image + ISR, no events, no generator
    REFUSED = {'cs2dz_image+raw-isr_no-fusion': 'the reference cannot run it: dacs.py:809 calls extract_feat(image=None, events=mixed_isr) '
                                                'without cfg, and encoder_decoder.py:703 then evaluates cfg.keys() on None',
               'cs2dz_image+d2n-isr': 'it needs pre-translated ISR files that no loader here produces'}
    IMAGE_TYPES = {'cs2dsec_image', 'cs2dz_image'}   # image-only: EventsEncoderDecoder, no events / ISR / fusion (_iteration_image)
    # ImageNet mean / std of the image normalisation (get_mean_std): the day -> night generator works on [-1, 1] images
    IMNET_MEAN, IMNET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

    def __init__(self, **cfg):
        super().__init__()
        if cfg.get('train_type') in self.REFUSED:
            raise ValueError(f"train_type {cfg['train_type']!r} is refused: {self.REFUSED[cfg['train_type']]}")
        if cfg.get('train_type') == self.SPLIT_TYPE and cfg['imnet_feature_dist_lambda'] > 0:
            raise ValueError(f"train_type {self.SPLIT_TYPE!r} with imnet_feature_dist_lambda > 0 is refused: the reference's feature-distance "
                             "step (dacs.py:568-575) ends in an assert for this train type")
        self.model = build_segmentor(deepcopy(cfg['model']))
        self.train_cfg = cfg['model'].get('train_cfg')
        self.test_cfg = cfg['model'].get('test_cfg')
        self.num_classes = cfg['model']['decode_head']['num_classes']
        self.local_iter = 0
        self.max_iters = cfg['max_iters']
        self.alpha = cfg['alpha']
        self.pseudo_threshold = cfg['pseudo_threshold']
        self.psweight_ignore_top = cfg['pseudo_weight_ignore_top']
        self.psweight_ignore_bottom = cfg['pseudo_weight_ignore_bottom']
        self.fdist_lambda = cfg['imnet_feature_dist_lambda']
        self.fdist_classes = cfg.get('imnet_feature_dist_classes')
        self.fdist_scale_min_ratio = cfg.get('imnet_feature_dist_scale_min_ratio')
        self.enable_fdist = self.fdist_lambda > 0
        if self.enable_fdist and self.fdist_classes is not None:
            # (downscale_label_ratio compares the cell ratios against it: the reference fails on None here as well)
            assert self.fdist_scale_min_ratio is not None, 'imnet_feature_dist_classes needs imnet_feature_dist_scale_min_ratio'
        self.mix = cfg['mix']
        assert self.mix == 'class'
        self.blur = cfg['blur']
        self.color_jitter_s = cfg['color_jitter_strength']
        self.color_jitter_p = cfg['color_jitter_probability']
        self.debug_img_interval = cfg['debug_img_interval']
        self.ema_model = build_segmentor(deepcopy(cfg['model']))
        self.train_type = cfg['train_type']
        assert self.train_type in self.SUPPORTED, f'train_type {self.train_type} is outside the accelerated hot path'
        self.image_only = self.train_type in self.IMAGE_TYPES
        self.split = self.train_type == self.SPLIT_TYPE
        self.forward_cfg = dict(cfg['forward_cfg'])
        self.img_self_res_reg = cfg.get('img_self_res_reg', 'no')
        assert not self.split or self.img_self_res_reg == 'no', "the split train type needs img_self_res_reg 'no' (dacs.py:538)"
        path = cfg.get('cyclegan_itrd2en_path', '')
        self.cyclegan_itrd2en = None
        if path and self.train_type in {'cs2dsec_image+events', 'cs2dsec_image+events_together'}:
            self.cyclegan_itrd2en = _frozen_generator(path)
        self.cyclegan_id2in = None
        path = cfg.get('cyclegan_id2in_path', '')
        if path and self.train_type == 'cs2dz_image':
            # dacs.py:105-113, :368-372: the source image through a frozen 3 -> 3 generator, [-1, 1] in and out:
            # G((x * std + mean - 0.5) / 0.5) / 2 + 0.5 - mean) / std -- both maps folded into the generator's first / last layer
            self.cyclegan_id2in = _frozen_generator(path, input_nc=3, output_nc=3)
            mean, std = torch.tensor(self.IMNET_MEAN), torch.tensor(self.IMNET_STD)
            self.cyclegan_id2in.set_io_affine(2.0 * std, 2.0 * (mean - 0.5), 0.5 / std, (0.5 - mean) / std)
        if cfg.get('cyclegan_light_path', '') and self.train_type == 'cs2dz_image':
            # (dacs.py:115-123 loads a LightNet whose use is commented out, :373-377 and encoder_decoder.py:364-367)
            raise ValueError("cyclegan_light_path: LightNet is not implemented (the reference loads it but never applies it); "
                             "leave cyclegan_light_path empty")
        self.imnet_model = None
        if self.enable_fdist and self.image_only:
            # dacs.py:234-241: for the image-only types a copy of the model config itself -- an EventsEncoderDecoder whose decode head is
            # built and never used; frozen as below
            self.imnet_model = _freeze(build_segmentor(deepcopy(cfg['model'])))
        elif self.enable_fdist:
            # dacs.py:234-242: an EncoderDecoder over the image backbone's config and the model's decode head (built, never used),
            # ImageNet weights from init_weights; frozen: no optimizer, no EMA, no gradient exchange sees it
            m = deepcopy(cfg['model'])
            self.imnet_model = _freeze(build_segmentor(dict(type='EncoderDecoder', backbone=m['backbone_image'], decode_head=m['decode_head'],
                                                            pretrained=m.get('pretrained'), train_cfg=m.get('train_cfg'),
                                                            test_cfg=m.get('test_cfg'))))
        self.debug_fdist_mask = self.debug_gt_rescale = None
        # ISR augmentations of the night-robustness recipe (dacs.py:125-129, :153-157): the noise bank lives on the device from here on
        bank = None
        if cfg.get('sky_mask') is not None:
            assert not self.image_only, 'sky_mask acts on the source ISR: the image-only train types have none'
            bank = ops.load_noise_bank(cfg['sky_mask'])
        self.register_buffer('sky_bank', bank, persistent=False)   # (a buffer: it moves with the module; not part of the state dict)
        self.isr_noise_dacs_type = cfg.get('isr_noise_dacs_type') or ''
        assert self.isr_noise_dacs_type in ops.ISR_NOISE_TYPES, f'isr_noise_dacs_type {self.isr_noise_dacs_type!r} not in {ops.ISR_NOISE_TYPES}'
        assert not (self.isr_noise_dacs_type and self.image_only), 'isr_noise_dacs_type acts on the mixed ISR: the image-only train types have none'
        # key of the kernel's noise generator; the per-iteration offset is the iteration counter, staged in the control block
        self.isr_noise_seed = torch.initial_seed() & (2 ** 63 - 1)
        self.mixed_image_to_mixed_isr = bool(cfg.get('mixed_image_to_mixed_isr'))
        self.isr_parms = {'val_range': (1, 10 ** 2), '_threshold': 0.04, '_clip_range': 0.2, 'shift_pixel': 3}
        # three-channel ISR of the mixed image: the flag (dacs.py:159-165, the 'dacs' preset) or `isr_parms` as a list of three dicts
        # under one value range; the flag together with isr_parms is refused as there (:167-168)
        self.isr3 = None
        if cfg.get('shift_3_channel'):
            assert not cfg.get('isr_parms'), 'shift_3_channel picks its own parameters: give it or isr_parms, not both'
            from .datasets import ISR3_PRESETS
            self.isr3 = [dict(p) for p in ISR3_PRESETS['dacs']]
        elif isinstance(cfg.get('isr_parms'), (list, tuple)):
            from .datasets import check_isr3
            self.isr3 = check_isr3(cfg['isr_parms'])
        elif cfg.get('isr_parms'):
            self.isr_parms = dict(cfg['isr_parms'])
        assert not (self.isr3 and self.image_only), 'a three-channel ISR acts on the mixed ISR: the image-only train types have none'
        # (the reference recomputes the ISR of the mixed image for its ISR types only, dacs.py:727; the image-only types have none)
        assert self.image_only or self.mixed_image_to_mixed_isr, 'configs/fusion/* recompute the ISR from the mixed image'
        self.isr_another_fusion = bool(cfg.get('isr_another_fusion'))
        self.fuse_both_ice_and_e = bool(cfg.get('fuse_both_ice_and_e'))
        self.without_events = bool(cfg.get('without_events'))
        self.without_isd = bool(cfg.get('without_isd'))
        self.isr_no_fusion = bool(cfg.get('isr_no_fusion'))
        rct = cfg.get('random_choice_thres', '')
        self.random_choice_thres = float(rct) if rct in {'0.25', '0.75', '0.5'} else 0.5
        self.shift_type = cfg.get('shift_type') or 'rightdown'
        assert self.shift_type in {'all', 'random', 'rightdown'}
        lfc = cfg.get('lambda_feature_consistency', -1)
        self.forward_cfg['lambda_feature_consistency'] = lfc if lfc != -1 else 0.25
        self._flat = None
        self._opt = None                   # the FlatAdamW whose flat store the teacher shares (attach_flat_store)
        self._graph, self._graphs = None, {}
        self._graph_warmup = None
        self._teacher_mode_set = False
        # switches that bench.py, the tests and tools/ set from outside
        self.fused_student_passes = True   # source + mixed samples as ONE student pass where the segmentor can (_iteration)
        self.early_student = True          # the EARLY-STUDENT schedule of _iteration (needs lane 'T')
        self.split_fused_targets = True    # split train type: both streams' targets from ops.split_mix_targets (else _mix_targets twice)
        self.graph_lanes = True            # the captured iteration runs on concurrency lanes ...
        self.graph_lane_set = None         # ... these (None: CMDA_LANES, else GRAPH_LANES)
        self.final_pass_grad_hook = None   # runtime.grad_ready_hook during the step's last backward pass (data-parallel drivers)
        self.inject_draws = None           # host decisions to use instead of _draw()'s
        self.last_draws = self.last_mix = None   # what the last iteration drew / mixed
        for p in self.ema_model.parameters():
            p.requires_grad_(False)

    # -- UDADecoratorFusion ------------------------------------------------------------------------------------------
    def get_model(self):
        return self.model

    def get_ema_model(self):
        return self.ema_model

    def extract_feat(self, img):
        return self.get_model().extract_feat(img)

    def encode_decode(self, img, events, **kw):
        return self.get_model().encode_decode(img, events, **kw)

    def simple_test(self, rescale=True, **kwargs):
        return self.get_model().simple_test(rescale, **kwargs)

    def predict(self, rescale=True, gt_semantic_seg=None, meter=None, **kwargs):
        return self.get_model().predict(rescale, gt_semantic_seg=gt_semantic_seg, meter=meter, **kwargs)

    def aug_test(self, *args, **kwargs):
        return self.get_model().aug_test(*args, **kwargs)

    def predict_aug(self, samples, gt_semantic_seg=None, meter=None):
        return self.get_model().predict_aug(samples, gt_semantic_seg=gt_semantic_seg, meter=meter)

    def get_imnet_model(self):
        return self.imnet_model

    def init_weights(self):
        self.model.init_weights()
        self.ema_model.init_weights()
        if self.imnet_model is not None:
            self.imnet_model.init_weights()   # the model's `pretrained` checkpoint lands here as well
            rt.refresh_frozen(self.imnet_model)

    # -- EMA teacher -----------------------------------------------------------------------------------------------------
    def attach_flat_store(self, opt):
        """Re-home the teacher's parameters into a flat buffer laid out like the student's (cmda_amd.optim.FlatAdamW),
        so that the EMA update is ONE kernel over 177.8 M floats."""
        offsets = {}
        flat_p = opt.flat_p
        base = flat_p.data_ptr()
        for n, p in self.model.named_parameters():
            offsets[n] = (p.data_ptr() - base) // 4
        ema_flat = torch.zeros_like(flat_p)
        from .optim import _slot_view
        student = dict(self.model.named_parameters())
        with torch.no_grad():
            for n, p in self.ema_model.named_parameters():
                off = offsets[n]
                view = _slot_view(ema_flat, off, student[n])   # same storage order as the student's slot (channels-last conv weights)
                view.copy_(p.data)
                p.data = view
        self._flat = (flat_p, ema_flat)
        self._opt = opt   # (an overlapped update -- FlatAdamW.overlap -- is waited for inside the iteration, see _iteration)
        # bf16 compute copies of the teacher in one flat mirror too, refreshed by ONE cast after each EMA update (without
        # it every teacher Linear weight is cast on its own: ~1100 extra launches per iteration)
        self._ema_bf16 = None
        if rt.compute_dtype() == torch.bfloat16 and ema_flat.is_cuda:
            self._ema_bf16 = torch.empty(ema_flat.numel(), dtype=torch.bfloat16, device=ema_flat.device)
            for n, p in self.ema_model.named_parameters():
                p._cmda_bf16 = _slot_view(self._ema_bf16, offsets[n], student[n])
            self._sync_ema_bf16()

    def _sync_ema_bf16(self):
        if getattr(self, '_ema_bf16', None) is not None:
            n = self._flat[1].numel()
            ops.permute4(self._flat[1], self._ema_bf16, (n, 1, 1, 1), (0, 1, 2, 3))

    @staticmethod
    def _ema_one(e, p, alpha):
        if e.data.is_contiguous() and p.data.is_contiguous():
            ops.ema_update(e.data.view(-1), p.data.view(-1), alpha)
        else:   # differently stored tensors (a channels-last student slot against a plain teacher tensor): by logical index
            e.data.mul_(alpha).add_(p.data, alpha=1.0 - alpha)

    def _init_ema_weights(self):
        if self._flat is not None:
            ops.ema_update(self._flat[1], self._flat[0], 0.0, mirror=getattr(self, '_ema_bf16', None))
        else:
            for e, p in zip(self.ema_model.parameters(), self.model.parameters()):
                self._ema_one(e, p, 0.0)
        rt.invalidate()

    def _update_ema(self, it):
        alpha_teacher = min(1 - 1 / (it + 1), self.alpha)
        if self._flat is not None:
            ops.ema_update(self._flat[1], self._flat[0], alpha_teacher, mirror=getattr(self, '_ema_bf16', None))
        else:
            for e, p in zip(self.ema_model.parameters(), self.model.parameters()):
                self._ema_one(e, p, alpha_teacher)
        rt.invalidate()

    # -- one UDA iteration ---------------------------------------------------------------------------------------------------
    def train_step(self, data_batch, optimizer, **kwargs):
        optimizer.zero_grad()
        log_vars = self(**data_batch)
        optimizer.step()
        # base.py:736-741: under data parallelism every logged scalar is its mean over the ranks (one small all-reduce)
        log_vars = reduce_log_vars(log_vars)
        log_vars.pop('loss', None)
        src = data_batch['source']
        n = src['image'].shape[0] if 'image' in src else data_batch['target']['warp_image'].shape[0]
        return dict(log_vars=log_vars, num_samples=n)

    def forward(self, **kwargs):
        return self.forward_train(**kwargs)

    def _choose_classes(self, labels):
        """get_class_masks (dacs_transforms.py:101-112): classes = unique over the WHOLE batch, ceil(n/2) drawn per
        sample with np.random.choice.  One small device->host read (<= 20 class ids), as in the reference.  Returns a CPU
        int64 [B, Kmax] tensor padded with -1 (Kmax fixed by num_classes, so the launch shapes never change)."""
        host = getattr(labels, '_cmda_classes', None)
        if host is not None and getattr(labels, '_cmda_classes_key', None) != (labels.data_ptr(), labels._version):
            host = None   # the label buffer was refilled in place after the loader attached its class set: recompute (dacs_transforms.py:103)
        if host is not None:
            # the loader took the class set on the host from the cropped labels before the H2D copy (datasets.CityscapesICDataset):
            # no device read, no sync, nothing to order
            classes = host
        elif labels.is_cuda and getattr(self, '_graph_warmup', None) is not None:
            # graph mode: the host runs an iteration ahead of the GPU, so the read goes through a side stream instead of draining
            # the main one -- ORDERED after the label's producer: the event the loader recorded behind its copy (`_cmda_ready`),
            # else everything enqueued so far on the current stream (safe for any producer; costs the run-ahead).  record_stream
            # keeps the caching allocator from recycling the buffer under the reader.
            side = getattr(self, '_side_stream', None) or torch.cuda.Stream(labels.device)
            self._side_stream = side
            ready = getattr(labels, '_cmda_ready', None)
            if ready is not None:
                side.wait_event(ready)
            else:
                side.wait_stream(torch.cuda.current_stream(labels.device))
            with torch.cuda.stream(side):
                classes = torch.unique(labels).cpu()
            labels.record_stream(side)
        else:
            classes = torch.unique(labels).cpu()
        n = classes.shape[0]
        k = int((n + n % 2) / 2)
        out = torch.full((labels.shape[0], self._kmax()), -1, dtype=torch.int64)
        for i in range(labels.shape[0]):
            pick = np.random.choice(n, k, replace=False)
            out[i, :k] = classes[torch.as_tensor(pick).long()]
        return out

    def _kmax(self):
        return (self.num_classes + 2) // 2   # labels 0..num_classes-1 plus the ignore index -> at most ceil((nc+1)/2) classes

    # -- host decisions of one iteration (everything random that the reference draws on the host) -------------------------------
    def _draw(self, day_label, H, W):
        """dacs.py:417 (events / ISR choice), :446-456 (strong_parameters), dacs_transforms.py:101-112 (class draw), and the
        per-sample kornia ColorJitter draws of strong_transform (one call per sample, dacs.py:721-724)."""
        B = day_label.shape[0]
        d = {}
        if self.image_only:
            d['choice'] = None   # (no events / ISR choice: the torch.rand of dacs.py:414-417 is in the events branch only)
        elif self.train_type in self.RAW_ISR_TYPES:
            d['choice'] = 0.0
        elif self.without_events:
            d['choice'] = -1.0
        elif self.without_isd:
            d['choice'] = 2.0
        else:
            d['choice'] = float(torch.rand(1))   # CPU generator: no device sync
        d['sky'] = d['isr_noise'] = None
        if self.sky_bank is not None:
            # dacs.py:431-434: one sky_mask_transform per sample, right behind the events / ISR choice.  With the loader's per-sample
            # sky counts the draws stop where the reference's early return stops them; without, all six are drawn (ops.draw_sky_mask)
            counts = self._sky_counts(day_label)
            d['sky'] = [ops.draw_sky_mask(self.sky_bank.shape[0], H, W, None if counts is None else counts[b]) for b in range(B)]
        d['color_jitter'] = random.uniform(0, 1)
        d['blur'] = random.uniform(0, 1) if self.blur else 0
        d['sigma'] = random.uniform(0.15, 1.15)
        d['classes'] = self._choose_classes(day_label)
        d['jitter'] = None
        if d['color_jitter'] > self.color_jitter_p:
            s_ = self.color_jitter_s
            lo = max(0.0, 1 - s_)
            d['jitter'] = [([int(v) for v in np.random.permutation(4)], random.uniform(lo, 1 + s_), random.uniform(lo, 1 + s_),
                            random.uniform(lo, 1 + s_), random.uniform(-s_, s_)) for _ in range(B)]
        if self.shift_type == 'random':
            cj = d['color_jitter']
            d['direction'] = _DIRECT[int(cj * 10) % 2][int(cj * 100) % 2]
        else:
            d['direction'] = self.shift_type
        if self.isr_noise_dacs_type:   # dacs.py:753-755: add_noise_on_isr's host draws, per sample, last in the mixing loop
            d['isr_noise'] = [ops.draw_isr_noise(self.isr_noise_dacs_type) for _ in range(B)]
        return d

    @staticmethod
    def _sky_counts(labels):
        """per-sample sky pixel counts the loader attached to the label tensor (datasets.CityscapesICDataset), None when absent or stale"""
        counts = getattr(labels, '_cmda_sky_counts', None)
        if counts is not None and getattr(labels, '_cmda_classes_key', None) != (labels.data_ptr(), labels._version):
            counts = None
        return counts

    # -- device-resident control block: what the host decided, in buffers whose addresses never change ----------------------
    def _control_block(self, dev, B, H, W):
        key = (str(dev), B, H, W)
        cb = getattr(self, '_ctl', None)
        if cb is not None and cb['key'] == key:
            return cb
        kx, ky = ops.blur_kernel_size(W), ops.blur_kernel_size(H)
        ndir = 4 if self.shift_type == 'all' else 2
        al = lambda n: (n + 3) // 4 * 4  # noqa: E731  (16-byte aligned sections)
        sizes = [('classes', 2 * B * self._kmax()), ('jitter', 8 * B), ('taps_x', kx), ('taps_y', ky), ('dirs', 2 * ndir), ('flags', 4)]
        if self.sky_bank is not None:
            sizes += [('sky_prm', 4 * B), ('sky_rows', B * H), ('sky_cols', B * W)]
        if self.isr_noise_dacs_type:
            sizes += [('noise_prm', 4 * B), ('offset', 2)]
        off, o = {}, 0
        for name, n in sizes:
            off[name] = (o, n)
            o += al(n)
        # ring of pinned staging buffers: the host may run several iterations ahead of the GPU (graph replay), so a buffer is
        # rewritten only after the copy that read it has executed (event per slot)
        nring = 4 if dev.type == 'cuda' else 1
        hosts = [torch.zeros(o, dtype=torch.int32).pin_memory() if dev.type == 'cuda' else torch.zeros(o, dtype=torch.int32)
                 for _ in range(nring)]
        devbuf = torch.zeros(o, dtype=torch.int32, device=dev)

        def views(buf):
            v = {n: buf[a:a + ln] for n, (a, ln) in off.items()}
            d = dict(classes=v['classes'].view(torch.int64).view(B, self._kmax()), jitter=v['jitter'].view(torch.float32).view(B, 8),
                     taps_x=v['taps_x'].view(torch.float32), taps_y=v['taps_y'].view(torch.float32),
                     dirs=v['dirs'].view(ndir, 2), jitter_on=v['flags'][0:1], blur_on=v['flags'][1:2])
            if 'sky_prm' in v:
                d.update(sky_prm=v['sky_prm'].view(B, 4), sky_rows=v['sky_rows'].view(B, H), sky_cols=v['sky_cols'].view(B, W))
            if 'noise_prm' in v:
                d.update(noise_prm=v['noise_prm'].view(B, 4), offset=v['offset'].view(torch.int64))
            return d
        self._ctl = dict(key=key, hosts=hosts, hviews=[views(h) for h in hosts], events=[None] * nring, slot=0, dev=devbuf,
                         d=views(devbuf), kx=kx, ky=ky)
        if self.isr3:   # a constant of the configuration: uploaded here, once, never inside a captured region
            self._ctl['d']['isr3_prm'] = ops.isr_multi_params(self.isr3, 'rightdown', dev)
        return self._ctl

    def _stage(self, cb, draws):
        """host decisions -> the device control block: ONE asynchronous copy per iteration"""
        slot = cb['slot']
        cb['slot'] = (slot + 1) % len(cb['hosts'])
        if cb['events'][slot] is not None:
            cb['events'][slot].synchronize()
        h = cb['hviews'][slot]
        h['classes'].copy_(draws['classes'])
        on = draws['jitter'] is not None
        h['jitter_on'][0] = int(on)
        if on:
            h['jitter'].copy_(ops.jitter_params(draws['jitter']))
        blur_on = draws['blur'] > 0.5
        h['blur_on'][0] = int(blur_on)
        if blur_on:
            h['taps_x'].copy_(ops.gaussian_taps(cb['kx'], draws['sigma']))
            h['taps_y'].copy_(ops.gaussian_taps(cb['ky'], draws['sigma']))
        h['dirs'].copy_(torch.tensor(ops.isr_dirs(draws['direction'], self.isr_parms['shift_pixel']), dtype=torch.int32))
        if 'sky_prm' in h:
            prm, rows, cols = ops.sky_mask_params(draws['sky'])
            h['sky_prm'].copy_(prm), h['sky_rows'].copy_(rows), h['sky_cols'].copy_(cols)
        if 'noise_prm' in h:
            h['noise_prm'].copy_(ops.isr_noise_params(draws['isr_noise']))
            h['offset'][0] = self.local_iter
        cb['dev'].copy_(cb['hosts'][slot], non_blocking=True)
        if cb['dev'].is_cuda:
            ev = cb['events'][slot] or torch.cuda.Event()
            ev.record()
            cb['events'][slot] = ev

    def _cfg_student(self, use_events):
        tt = self.train_type
        if tt == 'cs2dsec_image+events_together':
            if self.fuse_both_ice_and_e:
                return dict(self.forward_cfg, fusion_all=True)
            if self.isr_another_fusion and not use_events:
                return dict(self.forward_cfg, fusion_isr=True)
        elif tt == 'cs2dsec_image+events':
            if self.isr_no_fusion and not use_events:
                return dict(self.forward_cfg, no_fusion=True)
            if self.isr_another_fusion and not use_events:
                return dict(self.forward_cfg, fusion_isr=True)
        return self.forward_cfg

    # -- ImageNet feature distance (dacs.py:318-354) -------------------------------------------------------------------------------
    def _fdist_targets(self, day_image, day_label):
        """the frozen encoder's stage-4 rows over the source image (eval mode: no DropPath; no saved state) and the rescaled label /
        class mask / device count of downscale_label_ratio (no mask when imnet_feature_dist_classes is None)"""
        imnet = self.imnet_model
        if imnet.training:
            imnet.eval()   # (calc_feat_dist, dacs.py:331)
        feats, _ = imnet.backbone.fwd(day_image, save=False)
        ft, h, w = feats[-1]
        fd = dict(ft=ft, h=h, w=w, rescaled=None, mask=None, count=None)
        if self.fdist_classes is not None:
            fd['rescaled'], fd['mask'], fd['count'] = ops.fdist_label_mask(day_label, h, w, self.fdist_classes, self.fdist_scale_min_ratio,
                                                                           self.num_classes)
        return fd

    def _fdist_hook(self, fd, student_rows, gscale, log_vars):
        """img_grad_hook of the student's backward pass: loss and gradient of lambda * masked_feat_dist, the gradient ADDED into the
        image encoder's stage-4 output gradient of the source rows (the student's source features: `student_rows()`)"""
        def hook(d_img):
            n = fd['ft'].shape[0]
            fs = student_rows()[:n]
            g = d_img[3]
            if g is None:
                g = d_img[3] = torch.zeros(n, fs.shape[1], dtype=fs.dtype, device=fs.device)
            loss, _ = ops.fdist_fwd_bwd(fs, fd['ft'], self.fdist_lambda, mask=None if fd['mask'] is None else fd['mask'].view(-1),
                                        count=fd['count'], gscale=gscale, grad=g[:n])
            log_vars['src.loss_imnet_feat_dist'] = loss.view(())
        return hook

    # -- the steps the fusion and the image-only iteration share -----------------------------------------------------------------
    def _ext_wait(self):
        """the stream lookup `rt.wait_external` takes when the optimizer update is overlapped (FlatAdamW.overlap), else None"""
        opt = self._opt
        return (lambda: getattr(opt, '_update_stream', None)) if (opt is not None and getattr(opt, 'overlap', False)) else None

    def _teacher_mode(self):
        if not self.ema_model.training or not self._teacher_mode_set:
            self.ema_model.train()          # BatchNorm keeps batch statistics (and updates its running stats) ...
            set_stochastic(self.ema_model, False)  # ... but DropPath / Dropout2d are off in the teacher (dacs.py:458-462)
            self._teacher_mode_set = True

    def _mix_targets(self, logits, lab, classes):
        """the teacher's 1/4-resolution logits -> pseudo-labels -> ClassMix'd labels / weights (dacs.py:653-711, :716-771 for the targets)"""
        B, H, W = lab.shape
        pseudo_label, _, count = ops.pseudo_label(logits, H, W, self.pseudo_threshold, want_prob=False)
        pseudo_weight = ops.pseudo_weight(count, B, H, W, self.psweight_ignore_top, self.psweight_ignore_bottom)
        gt_pixel_weight = torch.ones(B, H, W, dtype=torch.float32, device=lab.device)
        mixed_lbl = ops.class_mix_label(lab, pseudo_label, lab, classes).view(B, 1, H, W)
        mixed_weight = ops.class_mix(gt_pixel_weight.view(B, 1, H, W), pseudo_weight.view(B, 1, H, W), lab, classes).view(B, H, W)
        return pseudo_label, count, mixed_lbl, mixed_weight

    def _split_targets(self, logits_image, logits_events, lab, classes):
        """the split train type's `_mix_targets`: (pseudo [2,B,H,W], count [2], mixed labels {'image', 'events'} [B,1,H,W], mixed weights
        {'image', 'events'} [B,H,W]); one class draw serves both streams (dacs.py:719-763)"""
        B, H, W = lab.shape
        if self.split_fused_targets:
            pseudo, count, mixed, weight = ops.split_mix_targets(logits_image, logits_events, lab, classes, self.pseudo_threshold,
                                                                 self.psweight_ignore_top, self.psweight_ignore_bottom)
        else:   # the composed sequence, per stream
            parts = [self._mix_targets(lg, lab, classes) for lg in (logits_image, logits_events)]
            pseudo, count = torch.stack([p[0] for p in parts]), torch.cat([p[1] for p in parts])
            mixed, weight = torch.stack([p[2].view(B, H, W) for p in parts]), torch.stack([p[3] for p in parts])
        return (pseudo, count, {'image': mixed[0].view(B, 1, H, W), 'events': mixed[1].view(B, 1, H, W)},
                {'image': weight[0], 'events': weight[1]})

    def _mixed_image(self, day_image, night_image, lab, classes, ctl):
        """ClassMix + strong augmentation (dacs.py:716-724; dacs_transforms.py:64-98, kornia semantics): the on/off gates and the
        per-sample parameters are read from the control block by the kernels"""
        mixed_img = ops.class_mix(day_image, night_image, lab, classes)
        if self.color_jitter_p < 1.0:
            ops.color_jitter_(mixed_img, ctl['jitter'], ctl['jitter_on'])
        if self.blur:
            ops.gaussian_blur_(mixed_img, ctl['taps_x'], ctl['taps_y'], ctl['blur_on'])
        return mixed_img

    @contextlib.contextmanager
    def _last_backward(self, dev):
        """around the step's LAST backward pass: gradients it reports final are final for the step, so a data-parallel driver may start
        their all-reduce underneath the rest of the pass (`final_pass_grad_hook` armed as runtime.grad_ready_hook, restored on exit)"""
        hook = self.final_pass_grad_hook
        if hook is not None and dev.type == 'cuda' and torch.cuda.is_current_stream_capturing() and rt._conc['seg'] is None:
            hook = None   # one monolithic capture cannot call out; the segmented capture records the hook as a host step
        prev = rt.grad_ready_hook
        try:
            if hook is not None:
                rt.grad_ready_hook = hook
            yield
        finally:
            rt.grad_ready_hook = prev

    def _two_passes(self, student, fwd_src, fwd_mix, keep_mix, rows4, fd, join_fd, one, log_vars):
        """the student's source and mixed step as two passes (the image-only types, and the fusion routes the joint pass does not
        cover): the mixed forward runs after the source forward (BatchNorm running statistics), on lane 'T' next to the source
        backward; the mixed backward follows the join (gradients accumulate).  fwd_src / fwd_mix: the argument tuples of
        `student.train_fwd`; keep_mix: what lane 'T' keeps alive for the mixed forward; rows4(saved, feats) -> the source pass's stage-4
        image rows (feature distance); join_fd: the feature-distance targets were made on lane 'T', which this route otherwise joins
        only behind the source backward."""
        # feature-consistency term of the `isr_no_fusion` route (encoder_decoder.py:822-823): loss and gradient come from ONE launch per
        # pass, inside the backward pass (`fc_sink`), so the forward passes leave it alone
        fc = len(fwd_src) > 3 and getattr(student, '_feat_consis_on', lambda cfg: False)(fwd_src[3])
        kw = dict(defer_feat_consis=True) if fc else {}
        loss, (losses, _, feats_src), saved_src = student.train_fwd(*fwd_src, **kw)
        log_vars['decode.loss_seg'], log_vars['decode.acc_seg'] = loss, losses['acc_seg']
        with rt.lane('T', *keep_mix):
            loss, (losses, _, _), saved_mix = student.train_fwd(*fwd_mix, **kw)
        log_vars['mix.decode.loss_seg'], log_vars['mix.decode.acc_seg'] = loss, losses['acc_seg']
        log_vars['loss'] = loss   # _parse_losses of the mixed step overwrites 'loss' (dacs.py:851-857)
        kw_src = kw_mix = {}
        if fc:
            def fc_src(l):
                log_vars['decode.loss_feat_consis'] = l.view(())

            def fc_mix(l, loss_seg=loss):   # _parse_losses sums every '*loss*' entry of the mixed step into 'loss'
                log_vars['mix.decode.loss_feat_consis'] = l.view(())
                log_vars['loss'] = ops.axpby(loss_seg.view(1), l, 1.0, 1.0).view(())
            kw_src, kw_mix = dict(fc_sink=fc_src), dict(fc_sink=fc_mix)
        fd_hook = None
        if fd is not None:
            if join_fd:
                rt.join_lanes('T')
            fd_hook = self._fdist_hook(fd, lambda: rows4(saved_src, feats_src), one, log_vars)
        student.train_bwd(saved_src, one, img_grad_hook=fd_hook, **kw_src)
        del saved_src, feats_src
        rt.join_lanes('T')
        with self._last_backward(one.device):
            student.train_bwd(saved_mix, one, **kw_mix)

    @staticmethod
    def _with_fdist(extras, fd):
        if fd is not None:
            extras.update(fdist_feat_imnet=fd['ft'], fdist_mask=fd['mask'], fdist_gt_rescale=fd['rescaled'], fdist_count=fd['count'])
        return extras

    # -- the device work of one iteration: no host reads, no host-dependent launch shapes (capturable: hipGraph segments) ----------
    def _iteration(self, src, tgt, ctl, use_events, teacher_second, direction):
        """dacs.py:397-860 minus the host decisions (`_draw`), the EMA update and the optimizer step.  `ctl` = device views of
        the control block; `teacher_second` = the teacher's second input (events or ISR, already chosen); `use_events` /
        `direction` only select code paths that are fixed per configuration (student inputs of 'cs2dsec_image+events')."""
        if self.image_only:
            return self._iteration_image(src, tgt, ctl)
        tt = self.train_type
        ext_wait = self._ext_wait()
        day_image, day_isr, day_label = src['image'], src['img_self_res'], src['label']
        day_events = night_events = None
        raw_isr = tt in self.RAW_ISR_TYPES
        if raw_isr:
            night_image = tgt['warp_image'] if 'warp_image' in tgt else tgt['image']
        else:
            night_image, night_events = tgt['warp_image'], tgt['events_vg']
        B, _, H, W = day_image.shape
        dev = day_image.device
        log_vars = {}
        self._teacher_mode()
        student, teacher = self.get_model(), self.get_ema_model()
        cfg_s = self._cfg_student(use_events)
        one = rt.ones1(dev)
        lab = day_label.view(B, H, W)
        classes = ctl['classes']
        if self.sky_bank is not None:
            # dacs.py:431-434, before anything reads the source ISR; out of place: the loader's buffers are reused
            day_isr = ops.sky_mask(lab, day_isr, self.sky_bank, ctl['sky_prm'], ctl['sky_rows'], ctl['sky_cols'])
        # Schedule.  The reference runs source step, teacher, mixing, mixed step one after the other (dacs.py:489-860), but the
        # only data dependencies are: mixing needs the teacher's pseudo-labels and the generator's events; the student's
        # gradients are the sum over both steps; its BatchNorm running statistics see the source step before the mixed step.
        # Round-5 schedule (lane 'T' off): teacher -> mixing, the generator queued on the side lane behind the teacher's event encoder,
        # then the student ONCE over source + mixed samples.  Default since round 6 (lanes 'T', 'Tenc', 'wq' on, uda.GRAPH_LANES): the
        # EARLY-STUDENT schedule below.  With the lanes switched off (eager launches) the same code simply runs in program order.

        def teacher_labels():
            """teacher forward -> pseudo-labels -> ClassMix'd labels / weights (dacs.py:653-711, :716-771 for the targets)"""
            if not raw_isr and self.fuse_both_ice_and_e:
                ema = teacher.encode_decode_lowres(night_image, night_events, tgt['warp_img_self_res'], dict(self.forward_cfg, fusion_all=True))
            elif not raw_isr and self.isr_another_fusion and not use_events:
                ema = teacher.encode_decode_lowres(night_image, teacher_second, test_cfg=dict(self.forward_cfg, fusion_isr=True))
            else:
                ema = teacher.encode_decode_lowres(night_image, teacher_second, test_cfg=self.forward_cfg)
            if self.split:   # dacs.py:628-651, :759-763: each stream's output gives that stream's targets
                return (ema,) + self._split_targets(ema['image_output'], ema['events_output'], lab, classes)
            return (ema,) + self._mix_targets(ema['fusion_output'], lab, classes)

        def mixed_inputs():
            """the mixed image and its ISR (dacs.py:716-771)"""
            mixed_img = self._mixed_image(day_image, night_image, lab, classes, ctl)
            gray = ops.isr_gray(mixed_img)
            if self.isr3:   # dacs.py:745-752: three parameter rows, direction 'rightdown' whatever shift_type says
                mixed_isr = ops.isr_multi(gray, self.isr3[0]['val_range'], ctl['isr3_prm'], 3)
            else:
                mixed_isr = ops.isr_from_gray(gray, self.isr_parms['val_range'], self.isr_parms['_threshold'],
                                              self.isr_parms['_clip_range'], self.isr_parms['shift_pixel'], direction, dirs_dev=ctl['dirs'])
            if self.isr_noise_dacs_type:   # dacs.py:753-755: channel 0 through add_noise_on_isr, the result on all three channels
                mixed_isr = ops.isr_noise(mixed_isr, ctl['noise_prm'], self.isr_noise_dacs_type, seed=self.isr_noise_seed,
                                          offset_dev=ctl['offset'])
            return mixed_img, mixed_isr

        # EARLY-STUDENT schedule (lane 'T' enabled): the student's forward pass needs the MIXED INPUTS, which depend on the source labels,
        # the class draw and the generator only -- the teacher's pseudo-labels enter at the loss (mixed label / weight).  So the teacher
        # runs on its own lane from the start of the iteration (its two encoders one after the other), the mixed image / ISR are built
        # on this lane at once, the generator on the side lane, and the student's encoders start as soon as the generator is done; lane
        # 'T' is joined in front of the decode head's loss (train_fwd_passes before_head).  The reference's order (teacher before the
        # mixed step, dacs.py:653-860) only matters through these data dependencies.
        fused = self.fused_student_passes and hasattr(student, 'train_fwd_passes')
        early = self.early_student and rt.lane_enabled('T') and fused
        # OVERLAPPED UPDATE (FlatAdamW.overlap): AdamW, the gradient clear and the EMA update of the step boundary run on the optimizer's
        # own stream; the part of the iteration that reads no trainable weight -- the mixed inputs and the frozen generator -- is enqueued
        # FIRST and runs underneath them, then this lane waits for that stream (`wait_external`), refreshes the weight copies and goes on.
        pre = early and ext_wait is not None and not raw_isr and self.cyclegan_itrd2en is not None
        day_events_pre = None
        if pre:
            mixed_img, mixed_isr = mixed_inputs()
            with rt.lane('enc', src['img_time_res'], independent=True):
                day_events_pre = self.cyclegan_itrd2en.forward_mean3(src['img_time_res'])
        if ext_wait is not None:
            rt.wait_external(ext_wait)
        rt.refresh(force=True)   # all re-laid-out weight copies follow this iteration's masters (first node without the overlapped update)
        fd = None
        if early:
            with rt.lane('T', night_image, teacher_second, lab, classes, *[v for v in tgt.values() if isinstance(v, torch.Tensor)],
                         *((day_image, day_label) if self.enable_fdist else ())):
                if self.enable_fdist:   # no dependency inside the iteration: ahead of the teacher on its lane (joined before the head)
                    fd = self._fdist_targets(day_image, day_label)
                ema, pseudo_label, count, mixed_lbl, mixed_weight = teacher_labels()
            if not pre:
                mixed_img, mixed_isr = mixed_inputs()
        else:
            # ---- teacher pseudo-labels (dacs.py:653-711) -------------------------------------------------------------------------
            with rt.lane('T', night_image, teacher_second, *[v for v in tgt.values() if isinstance(v, torch.Tensor)]):
                ema, pseudo_label, count, mixed_lbl, mixed_weight = teacher_labels()
                mixed_img, mixed_isr = mixed_inputs()
            if self.enable_fdist:   # (this lane: the two-pass route's source backward reads it before lane 'T' is joined)
                fd = self._fdist_targets(day_image, day_label)

        # ---- Image Motion-Extractor (dacs.py:400-404), frozen, no grad ------------------------------------------------------------
        if not raw_isr:
            if self.cyclegan_itrd2en is not None:
                # frozen weights, static input: queued behind the teacher's event encoder on the side lane, next to the
                # teacher's fusion / decoder / pseudo-label / mixing work on this one
                # (EARLY-STUDENT: letting the image encoder start before the generator is done -- generator, event mix and event encoder on
                # the side lane without the join -- measured the same, 52.22 against 52.25 ms over three alternating runs: not kept)
                if day_events_pre is not None:
                    day_events = day_events_pre
                else:
                    with rt.lane('enc', src['img_time_res'], independent=True):
                        day_events = self.cyclegan_itrd2en.forward_mean3(src['img_time_res'])
                rt.join_lanes('enc')
            else:
                day_events = src['img_time_res']
        mixed_events = None
        if day_events is not None:
            if early:
                mixed_events = ops.class_mix(day_events, night_events, lab, classes)
            else:
                with rt.lane('T', day_events):
                    mixed_events = ops.class_mix(day_events, night_events, lab, classes)

        # ---- student inputs: source (dacs.py:489-523) and mixed (dacs.py:820-860) ---------------------------------------------------
        if raw_isr:
            in_src = {'image': day_image, 'events': day_isr}
            in_mix = {'image': mixed_img, 'events': mixed_isr}
        elif tt == 'cs2dsec_image+events_together':
            in_src = {'image': day_image, 'events': day_events, 'img_self_res': day_isr}
            in_mix = {'image': mixed_img, 'events': mixed_events, 'img_self_res': mixed_isr}
        else:
            in_src = {'image': day_image, 'events': day_events if use_events else day_isr}
            in_mix = {'image': mixed_img, 'events': mixed_events if use_events else mixed_isr}

        if fused and student._joint_ok(in_src['image'], in_src['events'], cfg_s):
            # ONE student pass over the source and the mixed samples: both steps run the same weights (the optimizer steps after
            # both, dacs.py:523 / :860 only accumulate gradients), so the 2B samples travel as one batch -- half the launches,
            # twice the rows per GEMM.  What is per step in the reference stays per step: BatchNorm batch statistics and the order
            # of the running-statistic updates (source first), the loss normalisation, DropPath / Dropout2d draws per sample.
            if not early:
                rt.join_lanes('T')
            ((l_src, d_src), (l_mix, d_mix)), saved = student.train_fwd_passes(
                [(in_src, day_label, None), (in_mix, mixed_lbl, mixed_weight)], cfg_s,
                before_head=(lambda: rt.join_lanes('T')) if early else None)
            # the student's stage-4 image features: block 0 of the joint buffer, the source pass's rows first
            fd_hook = self._fdist_hook(fd, lambda: saved[5][3][0], one, log_vars) if fd is not None else None
            log_vars['decode.loss_seg'], log_vars['decode.acc_seg'] = l_src, d_src['acc_seg']
            log_vars['mix.decode.loss_seg'], log_vars['mix.decode.acc_seg'] = l_mix, d_mix['acc_seg']
            log_vars['loss'] = l_mix   # _parse_losses of the mixed step overwrites 'loss' (dacs.py:851-857)
            with self._last_backward(dev):   # the only backward pass of the iteration
                student.train_bwd(saved, one, img_grad_hook=fd_hook)
            del saved
        else:
            # the source pass's stage-4 image rows: the joint buffer's block 0, or the image encoder's own output; under EARLY-STUDENT
            # the frozen encoder ran on lane 'T'
            self._two_passes(student, (in_src, day_label, None, cfg_s), (in_mix, mixed_lbl, mixed_weight, cfg_s), (),
                             lambda saved, feats: feats[3][0] if saved[0] == 'joint' else feats['f_image'][3][0],
                             fd, early, one, log_vars)
        extras = dict(mixed_img=mixed_img, mixed_lbl=mixed_lbl, mixed_isr=mixed_isr, pseudo_weight=mixed_weight,
                      pseudo_label=pseudo_label, classes=classes, mixed_events=mixed_events, day_events=day_events,
                      teacher_logits=ema, pseudo_count=count)
        if self.split:   # per stream: the plain keys carry the image stream's, `*_events` the events stream's
            extras.update(mixed_lbl=mixed_lbl['image'], mixed_lbl_events=mixed_lbl['events'], pseudo_weight=mixed_weight['image'],
                          pseudo_weight_events=mixed_weight['events'], pseudo_label=pseudo_label[0], pseudo_label_events=pseudo_label[1],
                          pseudo_count=count[0:1], pseudo_count_events=count[1:2])
        if self.sky_bank is not None:
            extras['day_isr'] = day_isr   # the sky-masked source ISR the student saw
        return log_vars, self._with_fdist(extras, fd)

    def _iteration_image(self, src, tgt, ctl):
        """the image-only iteration ('cs2dsec_image' / 'cs2dz_image'; dacs.py:363-377, :467-468, :569-570, :597-600, :701-791): the
        same host / device split, the same step boundary and the same shared steps as `_iteration`.  Schedule: the frozen generator
        (cs2dz_image) first -- it reads no trainable weight, so it runs underneath an overlapped optimizer update; then the teacher,
        its pseudo-labels / weights and the feature-distance targets on lane 'T' beside the mixed image on this lane; then the
        student's two passes (`_two_passes`)."""
        ext_wait = self._ext_wait()
        day_image, day_label = src['image'], src['label']
        night_image = tgt['warp_image'] if 'warp_image' in tgt else tgt['image']
        B, _, H, W = day_image.shape
        log_vars = {}
        self._teacher_mode()
        student, teacher = self.get_model(), self.get_ema_model()
        one = rt.ones1(day_image.device)
        lab = day_label.view(B, H, W)
        classes = ctl['classes']
        if self.cyclegan_id2in is not None:
            # dacs.py:368-372: the translated image replaces the source image for the source step, the feature distance and the mixing
            day_image = self.cyclegan_id2in(day_image)
        if ext_wait is not None:
            rt.wait_external(ext_wait)
        rt.refresh(force=True)   # all re-laid-out weight copies follow this iteration's masters
        fd = None
        with rt.lane('T', night_image, day_image, day_label, lab, classes):
            if self.enable_fdist:
                fd = self._fdist_targets(day_image, day_label)
            ema = teacher.encode_decode_lowres(night_image)
            pseudo_label, count, mixed_lbl, mixed_weight = self._mix_targets(ema, lab, classes)
        mixed_img = self._mixed_image(day_image, night_image, lab, classes, ctl)
        # (the frozen encoder ran on lane 'T': joined before the source backward when the feature distance is on)
        self._two_passes(student, (day_image, day_label, None), (mixed_img, mixed_lbl, mixed_weight), (mixed_img,),
                         lambda saved, feats: feats[3][0], fd, True, one, log_vars)
        extras = dict(mixed_img=mixed_img, mixed_lbl=mixed_lbl, pseudo_weight=mixed_weight, pseudo_label=pseudo_label, classes=classes,
                      teacher_logits=ema, pseudo_count=count, day_image=day_image)
        return log_vars, self._with_fdist(extras, fd)

    # -- hipGraph replay of the iteration ------------------------------------------------------------------------------------------
    def enable_graph(self, warmup_iters=2):
        """Capture `_iteration` after `warmup_iters` eager iterations -- as a chain of linear hipGraph segments replayed on the
        concurrency lanes' streams (runtime.SegmentedCapture) -- and replay it from then on: at the reference's 2+2 samples per
        GPU the eager step is bound by the host's launch rate, not by the GPU.  Only the EMA update, the control-block copy and
        the optimizer step stay outside."""
        self._graph_warmup = warmup_iters
        self._graph, self._graphs = None, {}

    def disable_graph(self):
        self._graph_warmup = None
        self._graph, self._graphs = None, {}

    def _capture(self, src, tgt, cb, use_events_struct, direction):
        dev = src['image'].device
        st_src = {k: v.clone() for k, v in src.items() if isinstance(v, torch.Tensor)}
        st_tgt = {k: v.clone() for k, v in tgt.items() if isinstance(v, torch.Tensor)}
        second = torch.empty_like(st_src['image'])
        ws_lanes = ('main', 'main/enc', 'main/T', 'main/T/enc')   # (the per-lane persistent workspaces exist before the capture starts)
        deferred.prealloc(dev, ws_lanes)
        torch.cuda.synchronize(dev)
        rt.refresh(force=True)   # every copy exists and is current before the capture starts
        lanes = self.graph_lane_set
        if lanes is None and os.environ.get('CMDA_LANES'):   # tuning: comma-separated lane set (runtime.set_concurrency)
            lanes = set(os.environ['CMDA_LANES'].split(','))
        if lanes is None:
            # the default set of the captured iteration (round 6, same-box A/B 55.4-55.9 -> 52.1-52.3 ms): 'enc' the two encoders side by
            # side; 'T' + 'Tenc' the EARLY-STUDENT schedule -- the teacher on two queues of its own from the start of the iteration, joined
            # in front of the decode head's loss; 'wq' the encoders' grouped weight gradients on those queues once the teacher is done
            lanes = set(GRAPH_LANES)
        seg = rt.SegmentedCapture(dev)
        g = seg
        if os.environ.get('CMDA_LANE_QUEUES', '1') != '0':   # every lane stream on a hardware queue of its own (runtime.prepare_lane_streams)
            en = lanes if lanes is not None else rt._conc['enabled']
            rt.prepare_lane_streams(dev, seg.main, ['main/' + n for n in sorted(en) if n in ('enc', 'T', 'hw')] +
                                    (['main/T/enc'] if 'T' in en and 'Tenc' in en else []))
            # (running an overlapped optimizer update on the TEACHER lane's stream -- idle at the step boundary, where the update's own stream
            # shares a hardware queue with the generator's lane -- let the generator start beside AdamW instead of behind it, and measured
            # 51.5-51.9 against 51.0-51.5 ms, three alternating runs: the generator then takes 3.7 instead of 2.3 ms.  Not kept.)
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        rt.set_concurrency(bool(self.graph_lanes), lanes, seg=seg)
        try:
            seg.begin(seg.main)
            out = self._iteration(st_src, st_tgt, cb['d'], use_events_struct, second, direction)
            rt.join_lanes()
            seg.end()
        finally:
            rt.set_concurrency(False)
        torch.cuda.synchronize(dev)
        key = (use_events_struct, direction, tuple(src['image'].shape), tuple(tgt_shape(tgt)))
        # one captured iteration per launch structure / batch shape, all kept: configurations whose structure follows a
        # per-iteration random choice ('cs2dsec_image+events', isr_another_fusion) alternate between two of them
        self._graphs[key] = self._graph = dict(graph=g, src=st_src, tgt=st_tgt, second=second, out=out, key=key)

    def forward_train(self, **kwargs):
        src, tgt = kwargs['source'], kwargs['target']
        tt = self.train_type
        day_label = src['label']
        B, _, H, W = src['image'].shape
        dev = src['image'].device
        if self.sky_bank is not None and tuple(self.sky_bank.shape[1:]) != (H, W):
            raise ValueError(f'sky_mask: the noise bank is {tuple(self.sky_bank.shape[1:])}, the source ISR {(H, W)}')
        draws = self.inject_draws or self._draw(day_label, H, W)
        self.last_draws = draws
        if not self.image_only:
            self.forward_cfg['isr_events_fusion_choice'] = draws['choice']
        use_events = not self.image_only and tt not in self.RAW_ISR_TYPES and draws['choice'] > self.random_choice_thres
        cb = self._control_block(dev, B, H, W)
        self._stage(cb, draws)
        opt = self._opt

        def boundary():
            """the step boundary's device work that precedes this iteration: the (possibly postponed) optimizer update, then the EMA
            teacher update -- with an overlapped update both on the optimizer's stream"""
            if opt is not None:
                opt.flush()
            with (opt._on_update_stream() if opt is not None else contextlib.nullcontext()):
                if self.local_iter == 0:
                    self._init_ema_weights()
                if self.local_iter > 0:
                    self._update_ema(self.local_iter)
        if self.image_only:
            second = None
        elif tt in self.RAW_ISR_TYPES:
            second = tgt['warp_img_self_res'] if 'warp_image' in tgt else tgt['night_isr']
        else:
            second = tgt['events_vg'] if (use_events or self.isr_no_fusion) else tgt['warp_img_self_res']
        # launch-shape-relevant part of the draws: only 'cs2dsec_image+events' / isr_another_fusion route differently by choice,
        # and only shift_type 'all' changes the number of ISR directions (the direction itself lives in the control block)
        struct_events = use_events if (tt == 'cs2dsec_image+events' or self.isr_another_fusion) else True
        ndir_key = 'all' if self.shift_type == 'all' else 'rightdown'
        graph_on = (getattr(self, '_graph_warmup', None) is not None and dev.type == 'cuda'
                    and self.local_iter >= self._graph_warmup)
        if graph_on:
            key = (struct_events, ndir_key, tuple(src['image'].shape), tuple(tgt_shape(tgt)))
            if key not in self._graphs:
                # (first replay, another launch structure, or another batch shape: the captured launches are shape-specific)
                boundary()
                boundary = lambda: None   # noqa: E731  (done: the capture synchronises the device)
                self._capture(src, tgt, cb, struct_events, ndir_key)
            G = self._graph = self._graphs[key]
            # the inputs are staged FIRST, the step boundary's HBM-bound passes (AdamW, EMA) are enqueued behind them on their own stream
            for k, v in G['src'].items():
                if v.data_ptr() != src[k].data_ptr():
                    v.copy_(src[k])
            for k, v in G['tgt'].items():
                if v.data_ptr() != tgt[k].data_ptr():
                    v.copy_(tgt[k])
            if second is not None:
                G['second'].copy_(second)
            boundary()
            G['graph'].replay()
            log_vars, extras = G['out']
        else:
            boundary()
            if opt is not None:
                opt.synchronize()   # eager launches: everything behind the (possibly overlapped) update
            log_vars, extras = self._iteration(src, tgt, cb['d'], struct_events, second, ndir_key)
        self.local_iter += 1
        self.last_mix = extras
        if extras.get('fdist_mask') is not None:   # calc_feat_dist's debug tensors (dacs.py:346-347), [B, 1, h, w] as there
            B_, h_, w_ = extras['fdist_mask'].shape
            self.debug_fdist_mask = extras['fdist_mask'].view(torch.bool).view(B_, 1, h_, w_)
            self.debug_gt_rescale = extras['fdist_gt_rescale'].view(B_, 1, h_, w_)
        return dict(log_vars)
