"""State of the concurrency lanes and of the work a backward pass defers, with the pinned host arenas its launch tables live in.
Bookkeeping only: the launches are in ops."""
import contextlib

import torch

from . import _lib as L

# The concurrency-lane stack (runtime.lane pushes and pops it).  Its top keys the workspaces and the deferred work below: lanes
# running side by side must not share a buffer, nor launch what another lane's producers may still be writing.
LANES = ['main']


def select(pending, lane):
    """the keys of `pending` that `lane` owns (every key for None): the lane and the lanes forked below it whose work was joined
    back (`<lane>/wgrad...`: the batched weight-gradient closures of runtime.lane_batch register theirs there)"""
    if lane is None:
        return list(pending)
    return [k for k in pending if k == lane or k.startswith(lane + '/wgrad')]


# ---- persistent per-lane workspaces: fp32, ZERO on entry by contract (whoever fills one leaves it zeroed), one per kind, device
# and lane (calls on one stream are ordered).  'ln': LayerNorm backward, made with the largest request seen on the device; 'zero':
# accumulation, at least 1 << 20 floats (1 << 22 preallocated); 'bn': fused BatchNorm statistics, at least 8 2048-channel layers'
_WS = {}
_LN_PEAK = {}


def _ws_floats(kind, device, n):
    if kind == 'ln':
        dkey = (device.type, device.index)
        n = _LN_PEAK[dkey] = max(_LN_PEAK.get(dkey, 64 * 2 * 1024), n)
        return n
    return max(n, 1 << 20 if kind == 'zero' else 8 * int(L.lib().cmda_bn_ws_floats(2048)))


def workspace(kind, device, n, make_in_capture=True):
    """the current lane's workspace of `kind`, at least n floats: made when missing or too small -- with make_in_capture=False,
    None instead inside a graph capture"""
    key = (kind, device.type, device.index, LANES[-1])
    ws = _WS.get(key)
    if ws is None or ws.numel() < n:
        if not make_in_capture and device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            return None
        ws = _WS[key] = torch.zeros(_ws_floats(kind, device, n), dtype=torch.float32, device=device)
    return ws


def prealloc(device, lanes):
    """make every kind's workspaces of the given lanes NOW, so that a graph capture never allocates one from its private pool"""
    for kind, n in (('ln', 0), ('zero', 1 << 22), ('bn', 0)):
        n = _ws_floats(kind, device, n)
        for lane in lanes:
            key = (kind, device.type, device.index, lane)
            if key not in _WS or _WS[key].numel() < n:
                _WS[key] = torch.zeros(n, dtype=torch.float32, device=device)


# ---- deferred work: registered inside ops.backward_scope (depth > 0), launched by ops.flush_deferred / gemm_flush_deferred ------
depth = 0
_STORES = []


class Store:
    """one kind of deferred work: pending {lane or queue key: work since its last launch}, plans (kept), regions (persistent)"""

    def __init__(self):
        self.pending, self.plans, self.regions = {}, {}, {}
        _STORES.append(self)


LN = Store()     # LayerNorm parameter gradients as per-block partial sums: {lane: {dgamma ptr: region}}
CONV = Store()   # convolution weight gradients in [Co, KH*KW*Ci] shadows: {lane: {grad ptr: shadow}}
GEMM = Store()   # queued weight-gradient GEMMs: {lane or queue key: [problem]}
TAIL = Store()   # closures postponed to the tail of the backward pass: {queue key: [fn]}


def reset():
    """drop what every store has pending (a backward pass that died half way)"""
    for s in _STORES:
        s.pending.clear()


def launch_plans(store, lane, make):
    """take the regions `lane` owns in `store`; yield per device (plan, one of its regions' tensors): the regions sorted by key,
    the plan cached under (device, keys) and made by make(device, regions) on first use"""
    taken, by_dev = {}, {}
    for k in select(store.pending, lane):
        taken.update(store.pending.pop(k))
    for key, r in taken.items():
        by_dev.setdefault(r[0].device, {})[key] = r
    for dev, regions in by_dev.items():
        keys = tuple(sorted(regions))
        plan = store.plans.get((dev, keys))
        if plan is None:
            plan = store.plans[(dev, keys)] = make(dev, [regions[k] for k in keys])
        yield plan, regions[keys[0]][0]


def ln_region(dgamma, dbeta, C):
    """the partial-sum workspace of the LayerNorm whose parameter gradients are dgamma / dbeta, registered on the current lane"""
    key = dgamma.data_ptr()
    r = LN.regions.get(key)
    if r is None or r[0].device != dgamma.device:
        nslots = L.lib().cmda_layernorm_slots()
        r = LN.regions[key] = (torch.zeros(nslots * 2 * C, dtype=torch.float32, device=dgamma.device), dgamma, dbeta, C, nslots)
    LN.pending.setdefault(LANES[-1], {})[key] = r
    return r[0]


def conv_shadow(grad, cols):
    """the zeroed fp32 [Co, cols] shadow of the conv weight gradient `grad`, registered on the current lane"""
    key = grad.data_ptr()
    r = CONV.regions.get(key)
    if r is None or r[0].device != grad.device or r[0].shape[1] != cols:
        r = CONV.regions[key] = (torch.zeros(grad.shape[0], cols, dtype=torch.float32, device=grad.device), grad)
    CONV.pending.setdefault(LANES[-1], {})[key] = r
    return r[0]


# Queue key of gemm(defer=True) and tail_defer (None: the current lane).  The decode head's weight gradients are queued under their
# own key when they are to run in the TAIL of the backward pass (segmentors.train_bwd): the per-stage flushes of the encoders'
# backward passes, which run on the same lane in between, must not launch them.
_QUEUE_KEY = None


@contextlib.contextmanager
def queue_under(key):
    global _QUEUE_KEY
    prev, _QUEUE_KEY = _QUEUE_KEY, key
    try:
        yield
    finally:
        _QUEUE_KEY = prev


def enqueue(problem):
    GEMM.pending.setdefault(_QUEUE_KEY or LANES[-1], []).append(problem)


def queued_tensors():
    """the tensors behind the current lane's queued problems: what a side lane that launches them must keep alive"""
    return [t for e in GEMM.pending.get(LANES[-1], ()) for t in e[1] if t is not None]


def tail_defer(fn):
    """run fn() now -- or, while a tail queue is open (`queue_under` inside a backward scope), with that queue (ops.run_tail)"""
    if _QUEUE_KEY is not None and depth > 0:
        TAIL.pending.setdefault(_QUEUE_KEY, []).append(fn)
    else:
        fn()


# ---- pinned host arenas ----------------------------------------------------------------------------------------------------------
_desc_arena = None


def host_table(desc, dev):
    """A small descriptor table (numpy array) the kernels read in place, in PINNED HOST memory on the GPU: a new set of layers may
    show up while a stream is capturing (the per-lane folds of a segmented capture differ from the eager iteration's), and neither
    a host-to-device copy nor an allocation is capturable -- a slice of an arena allocated up front, which never rewinds, is."""
    global _desc_arena
    raw = torch.from_numpy(desc.reshape(-1).view('u1').copy())
    if dev.type != 'cuda':
        return raw
    if _desc_arena is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('descriptor arena: run one eager backward pass before capturing')
        _desc_arena = [torch.empty(16 << 20, dtype=torch.uint8, pin_memory=True), 0]
    buf, lo = _desc_arena
    if lo + raw.numel() > buf.numel():
        raise RuntimeError('descriptor arena exhausted')
    tab = buf[lo:lo + raw.numel()]
    tab.copy_(raw)   # host-to-host
    _desc_arena[1] = lo + (raw.numel() + 63) // 64 * 64
    return tab


# The grouped GEMM launches' tables (plain CPU tensors under the emulator).  The MAIN arena holds every plan made before or inside a
# capture: a captured graph re-runs the upload kernel of its plans on every replay, so its slices are never reused.  Once a capture
# has pinned plans, EAGER plans made afterwards (operand pointers that differ from the captured ones) live in a RECYCLABLE arena,
# rewound (one sync, un-captured plans dropped) when it fills: pinned host memory stays bounded at two arenas (one
# retired 192 MB arena per exhaustion before).  'recycles' counts the rewinds.
GEMM_ARENA_BYTES = 192 << 20
GEMM_EAGER_ARENA_BYTES = 64 << 20
GEMM_ARENAS = {'main': None, 'eager': None, 'pinned_plans': False, 'recycles': 0}


def gemm_plan(key, dev, ws_bytes):
    """the cached plan [host table, device table, bytes, captured, recyclable] of a grouped launch and whether its table must be
    uploaded; ws_bytes(): the table's size, asked when a plan is made"""
    capturing = dev.type == 'cuda' and torch.cuda.is_current_stream_capturing()
    plan = GEMM.plans.get(key)
    # (a plan made eagerly in the recyclable arena is rebuilt in the main one for a capture: its graph needs a slice that stays)
    new = plan is None or (capturing and plan[4])
    if new:
        nbytes = ws_bytes()
        size = (max(nbytes, 16) + 255) // 256 * 256
        pin = dev.type == 'cuda'
        recyclable = GEMM_ARENAS['pinned_plans'] and not capturing
        if recyclable:
            a = GEMM_ARENAS['eager']
            if a is None or a[0].numel() < size:
                a = GEMM_ARENAS['eager'] = [torch.empty(max(GEMM_EAGER_ARENA_BYTES, size), dtype=torch.uint8, pin_memory=pin), 0]
            if a[1] + size > a[0].numel():
                if pin:
                    torch.cuda.synchronize(dev)   # every upload that read the eager arena has run
                GEMM.plans = {k: v for k, v in GEMM.plans.items() if v[3]}
                a[1] = 0
                GEMM_ARENAS['recycles'] += 1
        else:
            a = GEMM_ARENAS['main']
            if a is None:
                if capturing:
                    raise RuntimeError('grouped-GEMM arena: run one eager backward pass before capturing')
                a = GEMM_ARENAS['main'] = [torch.empty(GEMM_ARENA_BYTES, dtype=torch.uint8, pin_memory=pin), 0]
            if a[1] + size > a[0].numel():
                if capturing or GEMM_ARENAS['pinned_plans']:
                    raise RuntimeError('grouped-GEMM arena exhausted by captured plans: raise deferred.GEMM_ARENA_BYTES')
                if pin:
                    torch.cuda.synchronize(dev)   # eager plans only: every upload that read the arena has run
                GEMM.plans.clear()
                a[1] = 0
        host = a[0][a[1]:a[1] + size]
        a[1] += size
        plan = GEMM.plans[key] = [host, torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev), nbytes, False, recyclable]
    if capturing:
        GEMM_ARENAS['pinned_plans'] = True
        plan[3] = True    # a captured graph replays this plan's upload + launch: its arena slice and device table stay
    return plan, int(new)
