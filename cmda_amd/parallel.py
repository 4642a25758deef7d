"""Data-parallel layer: one process per GPU, gradients averaged with RCCL over xGMI (torch.distributed backend 'nccl'
IS RCCL on ROCm).  Replaces the reference's mmcv MMDistributedDataParallel scaffolding (mmseg/core/ddp_wrapper.py:70-89,
mmseg/apis/train.py:64-81), which never arms its reducer because DACS calls the wrapped module directly (SURVEY.md
section 0).

Design for MI355X: the student's gradients already live in ONE contiguous fp32 buffer (cmda_amd.optim.FlatAdamW), so
the exchange is a handful of large collectives on contiguous memory instead of ~1100 per-tensor hooks.  xGMI is
point-to-point (7 links x ~153 GB/s per GPU): large buckets keep every link busy, and the optional bf16 wire format
halves the bytes (177.8 M gradients = 711 MB fp32 / 356 MB bf16); each bucket is exchanged as reduce-scatter + all-gather
(every link carries 1/world of the bucket in each phase).  Buckets are issued on a side HIP stream so the
collective of bucket k overlaps the cast of bucket k+1; per-rank BatchNorm statistics, ClassMix class draws and the
pseudo-weight stay rank-local exactly as in the reference's batch-2 step.
"""
import os

import torch
import torch.distributed as dist


def init_distributed(backend=None):
    """Reads RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* (torchrun).  Returns (rank, local_rank, world)."""
    rank = int(os.environ.get('RANK', 0))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    if world > 1 and not dist.is_initialized():
        if backend is None:
            backend = 'nccl' if torch.cuda.is_available() else 'gloo'
        kw = {}
        if backend == 'nccl':
            torch.cuda.set_device(local_rank)
            kw['device_id'] = torch.device('cuda', local_rank)
        dist.init_process_group(backend, **kw)
    return rank, local_rank, world


def shard_range(total, rank, world):
    """Contiguous shard [lo, hi) of `total` samples for `rank` (rank r of a global batch gets pairs [2r, 2r+1])."""
    per = total // world
    assert per * world == total, 'global batch must divide evenly over the ranks'
    return rank * per, (rank + 1) * per


def reduce_log_vars(log_vars, group=None):
    """`_parse_losses`' distributed tail (mmseg/models/segmentors/base.py:736-741): every log scalar becomes its MEAN over the
    ranks (`dist.all_reduce(loss_value.div_(world))`).  The reference issues one all-reduce per scalar with a host sync each;
    here the scalars of a step travel as ONE small fp32 vector (the tail of the gradient exchange) and stay
    device tensors.  No-op (same dict) without an initialised process group or at world size 1.  Every rank must pass the same
    keys in the same order (it does: the keys are a function of the configuration)."""
    if not (dist.is_available() and dist.is_initialized()):
        return log_vars
    world = dist.get_world_size(group)
    if world <= 1 or not log_vars:
        return log_vars
    keys = list(log_vars.keys())
    vals = [log_vars[k] if isinstance(log_vars[k], torch.Tensor) else torch.tensor(float(log_vars[k])) for k in keys]
    dev = next((v.device for v in vals if v.is_cuda), vals[0].device)
    vec = torch.stack([v.detach().float().reshape(-1)[0].to(dev) for v in vals])
    vec.div_(world)
    dist.all_reduce(vec, group=group)
    out = type(log_vars)()
    for i, k in enumerate(keys):
        out[k] = vec[i].reshape(vals[i].shape) if vals[i].dim() else vec[i]
    return out


def broadcast_bn_buffers(model, src=0, group=None):
    """DistEvalHook._do_evaluate's first step (mmseg/core/evaluation/eval_hooks.py:92-100): DDP does not synchronise BatchNorm's
    running statistics, and in this recipe they really differ between ranks (every rank's decoder sees its own samples), so before
    a distributed evaluation rank `src`'s running_mean / running_var are broadcast to every rank -- all ranks then score the SAME
    model.  The reference issues two broadcasts per BatchNorm layer; here all statistics of the model travel as ONE flat fp32
    vector.  Returns the number of BatchNorm layers synchronised (0 without an initialised group / at world size 1)."""
    bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.track_running_stats
           and m.running_mean is not None]
    if not bns or not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) <= 1:
        return 0
    bufs = [b for m in bns for b in (m.running_var, m.running_mean)]
    flat = torch.cat([b.detach().reshape(-1).float() for b in bufs])
    dist.broadcast(flat, src, group=group)
    off = 0
    for b in bufs:
        n = b.numel()
        b.copy_(flat[off:off + n].view_as(b))
        off += n
    return len(bns)


def distributed_evaluate(model, samples, num_classes, ignore_index=255, nan_to_num=None, group=None, predict=None,
                         label_map=None, reduce_zero_label=False, force=False, on_device=False):
    """Distributed evaluation of the segmentor: `DistEvalHook._do_evaluate` (mmseg/core/evaluation/eval_hooks.py:86-121) +
    `multi_gpu_test` (mmseg/apis/test.py:216-274) + the dataset's mIoU (`mmseg/core/evaluation/metrics.py:89-125`).

    Order of the reference kept: (1) rank 0's BatchNorm running statistics are broadcast (`broadcast_bn_buffers`), (2) every rank scores
    its share of `samples` with `model.simple_test(rescale=True, ...)` in eval mode -- sample i belongs to rank i % world, the order a
    non-shuffling DistributedSampler deals them in; the sampler's wrap-around padding is what `collect_results` cuts off again, so it
    is not produced here --, (3) the results meet.  The reference ships every rank's full-resolution label maps to rank 0 (pickled
    through a tmpdir or an all-gather of byte tensors); here each rank folds its maps into the four per-class area histograms (on
    the device the predictor returned them on: the default `simple_test` hands back host label maps) and ONE all-reduce of
    4 x num_classes float64 sums them: same totals, ~600 bytes on the wire instead of H x W per image.  The vector that meets is
    moved to ONE device on every rank first -- the model's device on RCCL (which has no CPU backend), the host elsewhere -- so a
    rank without samples and a rank with host-side histograms agree.
    Every rank returns the same dict (aAcc, mIoU, mAcc, IoU[C], Acc[C]).  force: run the collectives even at world size 1 (tests).

    samples: a sequence of dicts, the keyword arguments of `simple_test` plus `gt_semantic_seg` (integer label map);
    predict(model, sample) -> label map replaces the default `model.simple_test(True, **inputs)[0]`.

    on_device: nothing leaves the GPU per image -- every rank calls `model.predict(True, gt_semantic_seg=gt, meter=meter, **inputs)`
    (one fused launch behind the network: labels and the confusion counters of a `metrics.ConfusionMeter`), then ONE int64
    all-reduce of the (num_classes + 1) x num_classes matrix and one `meter.compute`.  A sample that carries `augs` (a list of
    keyword dicts, one per view of a multi-scale / flip test) instead of inputs is scored through
    `model.predict_aug(augs, gt_semantic_seg=gt, meter=meter)`; test_cfg.mode 'slide' needs nothing here, it arrives through
    `predict`.  The label remappings stay host-side: `label_map` / `reduce_zero_label` raise with it."""
    from . import metrics
    if on_device:
        if label_map or reduce_zero_label:
            raise ValueError('distributed_evaluate: label_map / reduce_zero_label are host-side remappings; not with on_device=True')
        if predict is not None:
            raise ValueError('distributed_evaluate: on_device=True scores through model.predict; not with a predict= hook')
    on = dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or force)
    rank, world = (dist.get_rank(group), dist.get_world_size(group)) if on else (0, 1)
    broadcast_bn_buffers(model, 0, group)
    was_training = model.training
    model.eval()
    if on_device:
        dev = next((p.device for p in model.parameters()), torch.device('cpu'))
        meter = metrics.ConfusionMeter(num_classes, ignore_index, device=dev)
        with torch.no_grad():
            for i in range(rank, len(samples), world):
                s = dict(samples[i])
                gt = s.pop('gt_semantic_seg')
                if 'augs' in s:      # the views of a multi-scale / flip test: one launch per view and one behind them
                    model.predict_aug(s['augs'], gt_semantic_seg=gt, meter=meter)
                else:
                    model.predict(True, gt_semantic_seg=gt, meter=meter, **s)
        if was_training:
            model.train()
        if on:
            if dist.get_backend(group) != 'nccl':   # (a host-only backend: the matrix meets there)
                meter.conf = meter.conf.cpu()
            meter.all_reduce(group)
        return meter.compute(nan_to_num)
    tot = None
    with torch.no_grad():
        for i in range(rank, len(samples), world):
            s = dict(samples[i])
            gt = s.pop('gt_semantic_seg')
            pred = predict(model, s) if predict is not None else model.simple_test(True, **s)[0]
            pred = torch.as_tensor(pred)
            gt = torch.as_tensor(gt).reshape(pred.shape)
            parts = metrics.intersect_and_union(pred, gt, num_classes, ignore_index, label_map, reduce_zero_label)
            tot = parts if tot is None else tuple(a + b for a, b in zip(tot, parts))
    if was_training:
        model.train()
    vec = torch.stack(tot).reshape(-1).double() if tot is not None else torch.zeros(4 * num_classes, dtype=torch.float64)
    if on:
        model_dev = next((p.device for p in model.parameters()), torch.device('cpu'))
        vec = vec.to(model_dev if dist.get_backend(group) == 'nccl' else torch.device('cpu'))
        dist.all_reduce(vec, group=group)
    inter, union, _, lab = vec.view(4, num_classes)
    out = {'aAcc': inter.sum() / lab.sum(), 'IoU': inter / union, 'Acc': inter / lab}
    if nan_to_num is not None:
        out = {k: torch.nan_to_num(v, nan=float(nan_to_num)) for k, v in out.items()}
    out['mIoU'], out['mAcc'] = torch.nanmean(out['IoU']), torch.nanmean(out['Acc'])
    return out


class GradAllReducer:
    """Mean all-reduce of a flat gradient buffer in large buckets.

    Two ways to drive it per step:
      * `all_reduce_mean()` after the backward pass (everything at once), or
      * `start_range(lo, hi)` as soon as a contiguous slice of the buffer is final (the backward pass reports finished
        stages through `runtime.grad_ready_hook`), then `finish()`: the collectives of the early slices run on the side
        stream underneath the rest of the backward pass; `finish()` reduces whatever was not started and joins.
    Every rank must issue the same ranges in the same order (it does: the schedule is a function of the model only)."""

    def __init__(self, flat_grad, bucket_elems=32 * 1024 * 1024, wire_dtype=torch.float32, group=None, force=False, exchange='auto',
                 virtual_ways=1):
        """exchange: 'auto' = reduce-scatter + all-gather on RCCL, all-reduce elsewhere; 'rs_ag' = the reduce-scatter + all-gather
        arithmetic on ANY backend (padding to per * world, mean on the owned shard, wire format, gather, copy-back): where the
        backend has no reduce_scatter_tensor (gloo: the CPU tests run this path at world 2 and 4) the collective itself is an
        all-reduce of the padded bucket of which the rank keeps its own shard; 'all_reduce' = never split.
        virtual_ways > 1 (single-rank runs with `force`, i.e. `bench.py --force-reducer` on one GPU): the bucket is laid out, padded and
        exchanged as for THAT many ranks -- per = ceil(n / ways), zero tail, one reduce_scatter_tensor / all_gather_into_tensor pair
        per virtual shard on the world-1 group -- so RCCL's own collectives run with the shard-sized views, dtypes and buffer
        aliasing of a multi-rank exchange on a box that has one GPU."""
        assert exchange in ('auto', 'rs_ag', 'all_reduce')
        self.flat = flat_grad
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.active = self.world > 1 or (force and dist.is_initialized())  # force: run the collectives even alone (testing)
        self.wire_dtype = wire_dtype
        self.bucket_elems = bucket_elems
        n = flat_grad.numel()
        self.buckets = [(s, min(n, s + bucket_elems)) for s in range(0, n, bucket_elems)]
        self.stream = torch.cuda.Stream() if flat_grad.is_cuda else None
        self._wire = None
        if wire_dtype != flat_grad.dtype:
            self._wire = torch.empty(min(n, bucket_elems), dtype=wire_dtype, device=flat_grad.device)
        # reduce-scatter + all-gather where the backend has them (RCCL); gloo (the CPU tests) keeps all_reduce
        native = bool(self.active and flat_grad.is_cuda and dist.get_backend(group) == 'nccl')
        self._rs_ag = bool(self.active and exchange != 'all_reduce' and (native or exchange == 'rs_ag'))
        self._native_rs = native
        if self._rs_ag:
            cap = min(n, bucket_elems) + self.world
            self._wire_rs = torch.empty(cap, dtype=wire_dtype, device=flat_grad.device)
            self._shard = torch.empty(-(-cap // self.world), dtype=wire_dtype, device=flat_grad.device)
        self._started = []  # [lo, hi) slices already issued this step
        self.ways = self.world if self.world > 1 else max(1, int(virtual_ways))
        if self._rs_ag and self.ways != self.world:
            cap = min(n, bucket_elems) + self.ways
            self._wire_rs = torch.empty(cap, dtype=wire_dtype, device=flat_grad.device)
            self._shard = torch.empty(-(-cap // self.ways), dtype=wire_dtype, device=flat_grad.device)

    def _reduce(self, lo, hi):
        inv = 1.0 / self.world
        for s in range(lo, hi, self.bucket_elems):
            e = min(hi, s + self.bucket_elems)
            seg = self.flat[s:e]
            if self._rs_ag:
                # RCCL: reduce-scatter + all-gather on the wire buffer.  xGMI is point-to-point (7 links per GPU): the direct
                # reduce-scatter keeps every link busy with 1/world of the bucket, the mean is taken on the owned shard only
                # (1/world of the multiplies), and the all-gather returns the averaged bucket.
                n = e - s
                per = -(-n // self.ways)
                w = self._wire_rs[:per * self.ways]
                w[:n].copy_(seg)
                if per * self.ways > n:
                    w[n:].zero_()
                shard = self._shard[:per]
                if self.ways == self.world:
                    self._reduce_scatter(shard, w, per)
                    shard.mul_(inv)
                    self._all_gather(w, shard, per)
                else:   # one rank standing in for `ways`: every virtual shard through the collectives of the world-1 group
                    for k in range(self.ways):
                        wk = w[k * per:(k + 1) * per]
                        self._reduce_scatter(shard, wk, per)
                        shard.mul_(inv)
                        self._all_gather(wk, shard, per)
                seg.copy_(w[:n])
            elif self._wire is not None:
                w = self._wire[:e - s]
                w.copy_(seg)
                dist.all_reduce(w, group=self.group)
                seg.copy_(w)
                seg.mul_(inv)
            else:
                dist.all_reduce(seg, group=self.group)
                seg.mul_(inv)

    def _reduce_scatter(self, shard, w, per):
        """shard <- sum over ranks of w[rank * per : (rank + 1) * per]"""
        if self._native_rs:
            dist.reduce_scatter_tensor(shard, w, group=self.group)
            return
        # stand-in for backends without the collective: all-reduce the padded bucket, keep the owned shard.  gloo has no bf16 sum:
        # a narrower wire format is summed in fp32 and rounded once, like RCCL's fp32-accumulating reduction.
        r = dist.get_rank(self.group)
        t = w.float() if w.dtype != torch.float32 else w.clone()
        dist.all_reduce(t, group=self.group)
        shard.copy_(t[r * per:(r + 1) * per])

    def _all_gather(self, w, shard, per):
        """w[r * per : (r + 1) * per] <- rank r's shard, for every r"""
        if self._native_rs:
            dist.all_gather_into_tensor(w, shard, group=self.group)
            return
        parts = [torch.empty(per, dtype=torch.float32 if shard.dtype != torch.float32 else shard.dtype, device=shard.device)
                 for _ in range(self.world)]
        dist.all_gather(parts, shard.float() if shard.dtype != torch.float32 else shard, group=self.group)
        for i, t in enumerate(parts):
            w[i * per:(i + 1) * per].copy_(t)

    def start_range(self, lo, hi):
        """Issue the mean all-reduce of flat[lo:hi] now (its gradients are final); returns immediately."""
        if not self.active or hi <= lo:
            return
        self._started.append((lo, hi))
        if self.stream is not None:
            self.stream.wait_stream(torch.cuda.current_stream())  # everything enqueued so far produced these gradients
            with torch.cuda.stream(self.stream):
                self._reduce(lo, hi)
        else:
            self._reduce(lo, hi)

    def finish(self):
        """Reduce every slice not yet started, then make the current stream wait for all of it."""
        if not self.active:
            return
        todo, pos = [], 0
        for lo, hi in sorted(self._started):
            if lo > pos:
                todo.append((pos, lo))
            pos = max(pos, hi)
        if pos < self.flat.numel():
            todo.append((pos, self.flat.numel()))
        self._started = []
        if self.stream is not None:
            self.stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.stream):
                for lo, hi in todo:
                    self._reduce(lo, hi)
            torch.cuda.current_stream().wait_stream(self.stream)
        else:
            for lo, hi in todo:
                self._reduce(lo, hi)

    def all_reduce_mean(self):
        self.finish()
