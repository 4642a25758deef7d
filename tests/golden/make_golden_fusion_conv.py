"""Generates tests/golden/fusion_caf.npz (+ fusion_caf_dx.npz, fusion_caf_eval.npz), fusion_af.npz and fusion_conv_keys.json from the
reference's OWN ConvertAvgFusion and AverageFusion (mmseg/models/fusion/convert_avg_fusion.py, average_fusion.py, imported unmodified
through tests/golden/ref_shim.py).
Runs only in the authoring container; only arrays and key lists are committed.  Usage: python tests/golden/make_golden_fusion_conv.py

The two modules need four names ref_shim does not provide; they are supplied here, after ref_shim.install():
mmcv.cnn.build_conv_layer -> nn.Conv2d, mmcv.cnn.build_norm_layer -> ('bn' + postfix, nn.BatchNorm2d),
mmcv.utils.parrots_wrapper._BatchNorm -> torch's _BatchNorm, mmseg.models.utils.ResLayer -> a dummy.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402
from weights import sample_grad, seeded_fill, seeded_randn  # noqa: E402

torch.set_num_threads(8)
DIMS, STRIDES = [64, 128, 320, 512], [4, 8, 16, 32]
SEED, B, H, W = 93, 2, 64, 128


def load_reference():
    ref_shim.install()
    import mmcv.cnn
    import mmcv.utils
    import mmcv.utils.parrots_wrapper
    mmcv.cnn.build_conv_layer = lambda cfg, *a, **k: nn.Conv2d(*a, **k)
    mmcv.cnn.build_norm_layer = lambda cfg, planes, postfix='': ('bn' + str(postfix), nn.BatchNorm2d(planes))
    mmcv.utils.parrots_wrapper._BatchNorm = nn.modules.batchnorm._BatchNorm
    sys.modules['mmseg.models.utils'].ResLayer = type('ResLayer', (nn.Sequential,), {})
    builder = ref_shim.load('mmseg.models.builder')
    sys.modules['mmseg.models'].builder = builder
    caf = ref_shim.load('mmseg.models.fusion.convert_avg_fusion')
    af = ref_shim.load('mmseg.models.fusion.average_fusion')
    return caf.ConvertAvgFusion, af.AverageFusion


def feats(tag, h=H, w=W, dtype=torch.float32):
    return [seeded_randn((B, c, h // s, w // s), SEED, f'{tag}{i}').to(dtype) for i, (c, s) in enumerate(zip(DIMS, STRIDES))]


def run_train(module, fi, fe, dys):
    """one train-mode forward and backward; returns outputs, input gradients, parameter gradients, buffers"""
    fi = [f.clone().requires_grad_(True) for f in fi]
    fe = [f.clone().requires_grad_(True) for f in fe]
    module.train()
    module.zero_grad()
    outs = module(fi, fe)
    sum((o * d.to(o.dtype)).sum() for o, d in zip(outs, dys)).backward()
    return (outs, [f.grad for f in fi], [f.grad for f in fe], {n: p.grad for n, p in module.named_parameters()},
            {n: b.clone() for n, b in module.named_buffers()})


def rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300)).item()


def fp32_within_bounds(cls, h, w, channels_last):
    """torch fp32 against torch float64 on the same input, no outlier allowance: the fp32 bounds tests/test_fusion_conv.py holds the
    kernels to (outputs 1e-4, dx 3e-4, parameter gradients 5e-4, running statistics 1e-4) are the reference's own to meet"""
    fi, fe = feats('i', h, w), feats('e', h, w)
    dys = [seeded_randn(f.shape, SEED + 1, f'dy{i}') for i, f in enumerate(fi)]
    m32, m64 = seeded_fill(cls(), SEED), seeded_fill(cls(), SEED).double()
    if channels_last:
        m32 = m32.to(memory_format=torch.channels_last)
        fi32 = [f.contiguous(memory_format=torch.channels_last) for f in fi]
        fe32 = [f.contiguous(memory_format=torch.channels_last) for f in fe]
    else:
        fi32, fe32 = fi, fe
    r32 = run_train(m32, fi32, fe32, dys)
    r64 = run_train(m64, [f.double() for f in fi], [f.double() for f in fe], dys)
    worst = {}
    for i in range(4):
        worst['out'] = max(worst.get('out', 0), rel(r32[0][i], r64[0][i]))
        worst['dx'] = max(worst.get('dx', 0), rel(r32[1][i], r64[1][i]), rel(r32[2][i], r64[2][i]))
    for n in r64[3]:
        worst['grad'] = max(worst.get('grad', 0), rel(r32[3][n], r64[3][n]))
    for n in r64[4]:
        if 'running' in n:
            worst['running'] = max(worst.get('running', 0), rel(r32[4][n], r64[4][n]))
    print(f'fp32 vs float64 at {h}x{w}, channels_last={channels_last}:', {k: f'{v:.2e}' for k, v in worst.items()})
    assert worst['out'] <= 1e-4 and worst['dx'] <= 3e-4 and worst['grad'] <= 5e-4 and worst['running'] <= 1e-4, worst


def main():
    CAF, AF = load_reference()
    for h, w in ((64, 128), (64, 96)):
        for cl in (False, True):
            fp32_within_bounds(CAF, h, w, cl)
    fi, fe = feats('i'), feats('e')
    dys = [seeded_randn(f.shape, SEED + 1, f'dy{i}') for i, f in enumerate(fi)]
    m = seeded_fill(CAF(), SEED)
    outs, di, de, grads, bufs = run_train(m, fi, fe, dys)
    arrs = {}
    for i in range(4):
        arrs[f'out{i}'], arrs[f'di{i}'], arrs[f'de{i}'] = outs[i], di[i], de[i]
    for n, g in grads.items():
        arrs['grad.' + n] = sample_grad(g)
    for n, b in bufs.items():
        arrs['bn.' + n] = b
    m.eval()
    with torch.no_grad():
        for i, o in enumerate(m(fi, fe)):
            arrs[f'eval{i}'] = o
    # three files, each under the 1 MiB a committed file may have: the train-mode outputs with the parameter-gradient fingerprints and
    # the buffers, the eight input gradients, the eval-mode outputs
    part = lambda k: '_dx' if k.startswith(('di', 'de')) else '_eval' if k.startswith('eval') else ''
    for suffix in ('', '_dx', '_eval'):
        np.savez_compressed(os.path.join(HERE, f'fusion_caf{suffix}.npz'),
                            **{k: v.detach().numpy() for k, v in arrs.items() if part(k) == suffix})
    with torch.no_grad():
        np.savez_compressed(os.path.join(HERE, 'fusion_af.npz'), **{f'out{i}': o.numpy() for i, o in enumerate(AF()(fi, fe))})
    with open(os.path.join(HERE, 'fusion_conv_keys.json'), 'w') as f:
        json.dump(sorted(m.state_dict().keys()), f, indent=0)
    print('wrote fusion_caf.npz', {k: tuple(v.shape) for k, v in arrs.items() if not k.startswith(('grad.', 'bn.'))})
    names = ('fusion_caf.npz', 'fusion_caf_dx.npz', 'fusion_caf_eval.npz', 'fusion_af.npz', 'fusion_conv_keys.json')
    print('sizes', {n: os.path.getsize(os.path.join(HERE, n)) for n in names})


if __name__ == '__main__':
    main()
