"""Kernel-level tests of the ISR augmentations (cmda_amd/csrc/isr_augment.hip, include/cmda_hip_ext3.h): sky mask, ISR noise with
explicit and with generated fields, the ABI's refusals.  The checker is a plain torch CPU fp32 restatement of the formulas of
mmseg/models/utils/dacs_transforms.py:134-171 and :186-211, written here."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from cmda_amd import _lib, ops
from conftest import check_le

SKY = 10


# ---- restatements ------------------------------------------------------------------------------------------------------------------
def sky_mask_ref(label, isr, bank, draws, enable=None):
    """per sample: (out [C,H,W], expansion [H,W], blur_w [H,W]) stacked over the batch"""
    outs, exps, bws = [], [], []
    for b, d in enumerate(draws):
        x = isr[b].clone()
        H, W = x.shape[-2:]
        sky = (label[b].view(H, W) == SKY).float()
        k = d['k']
        if int(sky.sum()) < 10 or (enable is not None and not enable[b]) or k % 2 == 0 or not 21 <= k <= 61:
            outs.append(x), exps.append(torch.zeros(H, W)), bws.append(torch.ones(H, W))
            continue
        S = F.avg_pool2d(sky[None, None], k, stride=1, padding=k // 2, divisor_override=1)[0, 0].round()   # integer window counts
        expansion = (S > 0).float()
        weight = S / float(k * k)
        weight = weight * (1 - sky)
        mx, mn = weight.max(), weight.min()
        wn = (weight - mn) / (mx - mn) if mx != mn else torch.zeros_like(weight)
        blur_w = 1 - torch.clamp(wn + d['lam'] * (wn != 0), min=0, max=1)
        noise = (bank[d['index']].float() / 128 - 1)[d['rows'].long()][:, d['cols'].long()]
        out = torch.clamp(x * (1 - sky) * blur_w + noise * expansion * d['intensity'], min=-1, max=1)
        outs.append(out), exps.append(expansion), bws.append(blur_w)
    return torch.stack(outs), torch.stack(exps), torch.stack(bws)


def isr_noise_ref(isr, draws, mode, fields, enable=None):
    outs = []
    for b, (blur, t1, t2, inten) in enumerate(draws):
        if enable is not None and not enable[b]:
            outs.append(isr[b].clone())
            continue
        x = isr[b, 0:1]
        if 'blur' in mode and blur:
            size = x.shape[1:]
            x = F.avg_pool2d(x[None], kernel_size=(2, 2))
            x = F.interpolate(x, size=size, mode='bilinear', align_corners=False)[0]
        if 'noise' in mode:
            x = x * (fields[0, b].abs() < t1)
            x = x + fields[2, b] * inten * (fields[1, b].abs() < t2)
            x = torch.clamp(x, min=-1, max=1)
        outs.append(x.repeat(isr.shape[1], 1, 1))
    return torch.stack(outs)


# ---- sky mask ----------------------------------------------------------------------------------------------------------------------
def _labels(H, W):
    """[corner touching two borders, interior blob, thin stripe, exactly 9 sky pixels, exactly 10, all sky]"""
    g = torch.Generator().manual_seed(5)
    lab = torch.randint(0, 19, (6, H, W), generator=g)
    lab[lab == SKY] = 11
    lab[0, :H // 3, :W // 2] = SKY
    lab[1, H // 3:H // 3 + 13, W // 4:W // 4 + 17] = SKY
    lab[2, H // 2, 3:W - 5] = SKY
    lab[3, 5, 4:13] = SKY
    lab[4, 5, 4:14] = SKY
    lab[5] = SKY
    return lab


def _sky_draws(n, H, W, ks, n_noise=2, seed=3):
    torch.manual_seed(seed)
    draws = [ops.draw_sky_mask(n_noise, H, W) for _ in range(n)]
    for d, k in zip(draws, ks):
        d['k'] = k
    return draws


def _run_sky(tgt, lab, isr, bank, draws, enable=None, debug=True, k_host=None):
    prm, rows, cols = ops.sky_mask_params(draws)
    en = None if enable is None else tgt.to(torch.tensor(enable, dtype=torch.int32))
    r = ops.sky_mask(tgt.to(lab), tgt.to(isr), tgt.to(bank), tgt.to(prm), tgt.to(rows), tgt.to(cols), enable=en, debug=debug, k_host=k_host)
    return tuple(t.cpu() for t in r) if debug else r.cpu()


@pytest.mark.parametrize('H,W', [(72, 104), (44, 70)])
@pytest.mark.parametrize('C,ldt', [(1, torch.uint8), (3, torch.int64)])
def test_sky_mask(tgt, H, W, C, ldt):
    lab = _labels(H, W).to(ldt)
    g = torch.Generator().manual_seed(H + C)
    isr = torch.rand(6, C, H, W, generator=g) * 2 - 1
    bank = torch.randint(0, 256, (2, H, W), generator=g, dtype=torch.uint8)
    # k = 21, 41, 61 on the three sky shapes (at 44 x 70 the k = 61 window is taller than the image), then 9 / 10 pixels and all sky
    draws = _sky_draws(6, H, W, [21, 41, 61, 33, 33, 61])
    out, ex, bw = _run_sky(tgt, lab, isr, bank, draws)
    ref, rex, rbw = sky_mask_ref(lab, isr, bank, draws)
    assert torch.equal(ex, rex), 'expansion'
    assert torch.equal(bw, rbw), 'blur_w'
    check_le(f'sky_mask out {H}x{W} C{C}', (out - ref).abs().max().item(), 1e-6)
    assert torch.equal(out[3], isr[3]), 'a sample with 9 sky pixels passes through bit for bit'
    assert not torch.equal(out[4], isr[4]), 'a sample with 10 sky pixels is transformed'
    assert rex[4].sum() > 0 and torch.isfinite(out).all()
    assert torch.equal(bw[5], torch.ones(H, W)) and torch.equal(ex[5], torch.ones(H, W)), 'all sky: wn = 0'
    assert out.abs().max() <= 1
    out2, ex2, bw2 = _run_sky(tgt, lab, isr, bank, draws)
    assert torch.equal(out, out2) and torch.equal(bw, bw2), 'two runs are bit-equal'


def test_sky_mask_from_unit_input(tgt):
    """expansion and blur_w recomputed from the output where isr = 1 and bank = 128 (noise 0): out = (1 - sky) * blur_w"""
    H, W = 44, 70
    lab = _labels(H, W)[:3]
    draws = _sky_draws(3, H, W, [21, 41, 61])
    out = _run_sky(tgt, lab, torch.ones(3, 1, H, W), torch.full((2, H, W), 128, dtype=torch.uint8), draws, debug=False)
    _, _, rbw = sky_mask_ref(lab, torch.ones(3, 1, H, W), torch.full((2, H, W), 128, dtype=torch.uint8), draws)
    assert torch.equal(out[:, 0], (1 - (lab == SKY).float()) * rbw)


def test_sky_mask_gate_and_in_place(tgt):
    H, W = 44, 70
    lab = _labels(H, W)[:3].to(torch.uint8)
    g = torch.Generator().manual_seed(1)
    isr = torch.rand(3, 3, H, W, generator=g) * 2 - 1
    bank = torch.randint(0, 256, (2, H, W), generator=g, dtype=torch.uint8)
    draws = _sky_draws(3, H, W, [21, 41, 61])
    out, ex, bw = _run_sky(tgt, lab, isr, bank, draws, enable=[1, 0, 1])
    ref, rex, rbw = sky_mask_ref(lab, isr, bank, draws, enable=[1, 0, 1])
    assert torch.equal(out[1], isr[1]), 'a closed gate leaves the sample alone'
    assert torch.equal(ex, rex) and torch.equal(bw, rbw)
    check_le('sky_mask gated out', (out - ref).abs().max().item(), 1e-6)
    prm, rows, cols = ops.sky_mask_params(draws)
    buf = tgt.to(isr.clone())
    ops.sky_mask(tgt.to(lab), buf, tgt.to(bank), tgt.to(prm), tgt.to(rows), tgt.to(cols), out=buf,
                 enable=tgt.to(torch.tensor([1, 0, 1], dtype=torch.int32)))
    assert torch.equal(buf.cpu(), out), 'out = isr gives the out-of-place result'


def test_draw_sky_mask_order():
    """the draws in the reference's order from the torch CPU generator; the early stop below 10 sky pixels"""
    H, W = 44, 70
    torch.manual_seed(11)
    d = ops.draw_sky_mask(5, H, W, sky_count=10)
    torch.manual_seed(11)
    k = int(torch.randint(21, 61, size=(1,)))
    lam = torch.empty(1).uniform_(0.1, 0.3).item()
    inten = torch.empty(1).uniform_(0.5, 1.2).item()
    idx = int(torch.randint(0, 5, size=(1,)))
    noise = torch.arange(H * W).view(H, W)
    for i in range(2):
        chunks = torch.split(noise, 8, dim=i)
        noise = torch.cat([chunks[j] for j in torch.randperm(len(chunks))], dim=i)
    after = torch.rand(1)
    assert (d['k'], d['lam'], d['intensity'], d['index']) == (k + 1 - k % 2, lam, inten, idx)
    assert torch.equal(torch.arange(H * W).view(H, W)[d['rows'].long()][:, d['cols'].long()], noise)
    torch.manual_seed(11)
    ops.draw_sky_mask(5, H, W)
    assert torch.equal(torch.rand(1), after), 'without a sky count all six draws are taken'
    torch.manual_seed(11)
    e = ops.draw_sky_mask(5, H, W, sky_count=9)
    got = torch.rand(1)
    torch.manual_seed(11)
    torch.randint(21, 61, size=(1,)), torch.empty(1).uniform_(0.1, 0.3), torch.empty(1).uniform_(0.5, 1.2)
    assert torch.equal(got, torch.rand(1)), 'below 10 sky pixels the draws stop after the third'
    assert torch.equal(e['rows'], torch.arange(H, dtype=torch.int32)) and e['k'] == d['k']


# ---- ISR noise ---------------------------------------------------------------------------------------------------------------------
def _noise_draws(B, mode, gates):
    torch.manual_seed(21)
    draws = [ops.draw_isr_noise(mode) for _ in range(B)]
    return [(g if 'blur' in mode else 0,) + d[1:] for d, g in zip(draws, gates)]


@pytest.mark.parametrize('H,W', [(64, 96), (45, 71)])
@pytest.mark.parametrize('mode', ['noise', 'blur', 'noise+blur'])
@pytest.mark.parametrize('C', [1, 3])
def test_isr_noise_explicit_fields(tgt, H, W, mode, C):
    B = 3
    g = torch.Generator().manual_seed(H * C)
    isr = torch.rand(B, C, H, W, generator=g) * 2 - 1
    fields = torch.randn(3, B, H, W, generator=g)
    draws = _noise_draws(B, mode, [1, 0, 1])
    enable = [1, 1, 0]
    out = ops.isr_noise(tgt.to(isr), tgt.to(ops.isr_noise_params(draws)), mode, fields=tgt.to(fields),
                        enable=tgt.to(torch.tensor(enable, dtype=torch.int32))).cpu()
    ref = isr_noise_ref(isr, draws, mode, fields, enable)
    check_le(f'isr_noise {mode} {H}x{W} C{C}', (out - ref).abs().max().item(), 1e-6)
    assert torch.equal(out[2], isr[2]), 'a closed gate copies the sample through'
    if 'noise' in mode:
        assert not torch.equal(out[1, 0], isr[1, 0])
    else:
        assert torch.equal(out[1, 0], isr[1, 0]), "mode 'blur' with the sample's blur gate off changes nothing"
    for c in range(1, C):
        assert torch.equal(out[:2, c], out[:2, 0]), 'channel 0 on every channel'


@pytest.mark.parametrize('H,W', [(64, 96), (45, 71)])
def test_isr_noise_generated_fields(tgt, H, W):
    B, mode, seed, offset = 2, 'noise+blur', 0x1234567890abcdef, 7
    g = torch.Generator().manual_seed(W)
    isr = tgt.to(torch.rand(B, 3, H, W, generator=g) * 2 - 1)
    prm = tgt.to(ops.isr_noise_params(_noise_draws(B, mode, [1, 0])))
    fields = ops.randn_fields(B, H, W, seed, offset, device=tgt.device)
    gen = ops.isr_noise(isr, prm, mode, seed=seed, offset=offset)
    assert torch.equal(gen, ops.isr_noise(isr, prm, mode, fields=fields)), 'generated mode == explicit mode fed with randn_fields'
    assert torch.equal(gen, ops.isr_noise(isr, prm, mode, seed=seed, offset=offset)), 'same (seed, offset) twice'
    assert torch.equal(fields, ops.randn_fields(B, H, W, seed, offset, device=tgt.device))
    # the device half of the offset adds to the host half (the staged iteration counter of the training step)
    offd = tgt.to(torch.tensor([4], dtype=torch.int64))
    assert torch.equal(fields, ops.randn_fields(B, H, W, seed, 3, offset_dev=offd))
    assert torch.equal(gen, ops.isr_noise(isr, prm, mode, seed=seed, offset=3, offset_dev=offd))
    assert not torch.equal(gen, ops.isr_noise(isr, prm, mode, seed=seed, offset=offset + 1)), 'another offset'
    assert not torch.equal(gen, ops.isr_noise(isr, prm, mode, seed=seed + 1, offset=offset)), 'another seed'
    assert not torch.equal(fields, ops.randn_fields(B, H, W, seed, offset + (1 << 32), device=tgt.device)), 'the high word counts'


def test_randn_fields_statistics(tgt):
    """N = 16384 per field: every bound is 5 standard deviations of the estimator under the null hypothesis (iid N(0, 1))"""
    H = W = 128
    N = H * W
    f = ops.randn_fields(2, H, W, 99, 0, device=tgt.device).cpu().double().view(3, 2, N)
    assert torch.isfinite(f).all()
    p = 0.6827
    for i in range(3):
        x = f[i, 0]
        check_le(f'field {i} |mean|', x.mean().abs().item(), 5 / math.sqrt(N))
        check_le(f'field {i} |var - 1|', abs(x.var().item() - 1), 5 * math.sqrt(2 / N))
        check_le(f'field {i} |share(|n| < 1) - 0.6827|', abs((x.abs() < 1.0).double().mean().item() - p), 5 * math.sqrt(p * (1 - p) / N))
    def corr(a, b):
        return ((a - a.mean()) * (b - b.mean())).mean().item() / (a.std().item() * b.std().item())
    for i, j in ((0, 1), (0, 2), (1, 2)):
        check_le(f'corr fields {i},{j}', abs(corr(f[i, 0], f[j, 0])), 5 / math.sqrt(N), strict=True)
    for i in range(3):
        check_le(f'corr samples, field {i}', abs(corr(f[i, 0], f[i, 1])), 5 / math.sqrt(N), strict=True)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_isr_augment_refusals(tgt):
    from cmda_amd._lib import c_i32, c_i64, ptr
    H, W, B = 24, 40, 2
    lab = tgt.to(torch.full((B, H, W), SKY, dtype=torch.uint8))
    isr = tgt.to(torch.zeros(B, 3, H, W))
    draws = _sky_draws(B, H, W, [21, 23])
    prm, rows, cols = (tgt.to(t) for t in ops.sky_mask_params(draws))
    bank = tgt.to(torch.zeros(2, H, W, dtype=torch.uint8))
    sentinel = 7.0
    out = tgt.to(torch.full((B, 3, H, W), sentinel))
    ws = tgt.to(torch.empty(_lib.lib().cmdax3_sky_mask_ws_bytes(B, H, W), dtype=torch.uint8))
    lib = _lib.lib()

    def sky(bank_=bank, k=None, C=3, out_=out, bh=None, bw=None, tag=_lib.U8):
        kc = (ctypes.c_int * B)(*k) if k is not None else None
        return lib.cmdax3_sky_mask(ptr(lab), c_i32(tag), ptr(isr), ptr(bank_), ptr(prm), ptr(rows), ptr(cols), None, ptr(out_), None,
                                   None, ptr(ws), kc, c_i32(B), c_i32(C), c_i32(H), c_i32(W), c_i32(bank_.shape[0]),
                                   c_i32(bank_.shape[1] if bh is None else bh), c_i32(bank_.shape[2] if bw is None else bw),
                                   _lib.stream_of(isr))
    SHAPE, DTYPE, UNSUP = -1, -2, -4
    assert sky(bank_=tgt.to(torch.zeros(2, H, W + 8, dtype=torch.uint8))) == SHAPE, 'a bank of the wrong size'
    assert sky(bank_=tgt.to(torch.zeros(2, H - 1, W, dtype=torch.uint8))) == SHAPE
    assert sky(k=[22, 23]) == SHAPE and sky(k=[21, 19]) == SHAPE and sky(k=[63, 21]) == SHAPE, 'even k / k outside 21..61'
    assert sky(C=2) == SHAPE and sky(C=4) == SHAPE, 'C outside {1, 3}'
    assert sky(tag=5) == DTYPE
    assert sky(out_=None) == UNSUP, 'a null output'
    assert sky(k=[21, 23]) == 0
    with pytest.raises(_lib.CmdaError):
        ops.sky_mask(lab, isr, bank, prm, rows, cols, out=out.fill_(sentinel), k_host=[21, 30])
    assert torch.equal(out.cpu(), torch.full((B, 3, H, W), sentinel)), 'a refused call writes nothing'
    # an invalid k that only the device knows: the sample passes through
    bad = prm.clone()
    bad[0, 0] = 22
    got = ops.sky_mask(lab, tgt.to(torch.rand(B, 3, H, W)), bank, bad, rows, cols, debug=True)
    assert torch.equal(got[2][0].cpu(), torch.ones(H, W)) and torch.equal(got[1][0].cpu(), torch.zeros(H, W))

    nprm = tgt.to(ops.isr_noise_params([(1, 1.2, 0.5, 0.2)] * B))

    def noise(C=3, out_=out, n=(None, None, None), src=isr):
        return lib.cmdax3_isr_noise(ptr(src), ptr(out_), ptr(n[0]), ptr(n[1]), ptr(n[2]), ptr(nprm), None, c_i32(B), c_i32(C), c_i32(H),
                                    c_i32(W), c_i32(1), c_i32(1), ctypes.c_uint64(1), c_i64(0), None, _lib.stream_of(isr))
    out.fill_(sentinel)
    assert noise(C=2) == SHAPE and noise(out_=None) == UNSUP and noise(out_=isr) == UNSUP
    assert noise(n=(tgt.to(torch.zeros(B, H, W)), None, None)) == UNSUP, 'some but not all of the fields'
    assert lib.cmdax3_randn_fields(None, c_i32(B), c_i32(H), c_i32(W), ctypes.c_uint64(1), c_i64(0), None, _lib.stream_of(isr)) == UNSUP
    assert lib.cmdax3_randn_fields(ptr(out), c_i32(B), c_i32(0), c_i32(W), ctypes.c_uint64(1), c_i64(0), None, _lib.stream_of(isr)) == SHAPE
    assert torch.equal(out.cpu(), torch.full((B, 3, H, W), sentinel)), 'a refused call writes nothing'


# ---- parity with the reference's own functions (tests/golden/isr_aug.npz, made by tests/golden/make_golden_isr_aug.py) ------------
def _golden():
    import os
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'isr_aug.npz'))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _expand(perm, n):
    chunks = torch.split(torch.arange(n, dtype=torch.int32), 8)
    return torch.cat([chunks[int(i)] for i in perm])


def _golden_sky_draw(z, s, H, W):
    k = int(z[f's{s}_sky_k_drawn'])
    return dict(k=k + 1 - k % 2, lam=z[f's{s}_sky_lambda'].item(), intensity=z[f's{s}_sky_intensity'].item(),
                index=int(z[f's{s}_sky_index']), rows=_expand(z[f's{s}_sky_row_perm'], H), cols=_expand(z[f's{s}_sky_col_perm'], W))


def test_draw_sky_mask_reproduces_the_reference_draws():
    z = _golden()
    for s in z['seeds'].tolist():
        H, W = z[f's{s}_isr'].shape[-2:]
        want = _golden_sky_draw(z, s, H, W)
        for count in (None, int((z[f's{s}_label'] == SKY).sum())):
            torch.manual_seed(s)
            d = ops.draw_sky_mask(z['bank'].shape[0], H, W, sky_count=count)
            assert (d['k'], d['lam'], d['intensity'], d['index']) == (want['k'], want['lam'], want['intensity'], want['index'])
            assert torch.equal(d['rows'], want['rows']) and torch.equal(d['cols'], want['cols'])


def test_kernels_reproduce_the_reference_outputs(tgt):
    z = _golden()
    seeds = z['seeds'].tolist()
    isr = torch.stack([z[f's{s}_isr'] for s in seeds])           # [2, 1, H, W]
    lab = torch.stack([z[f's{s}_label'][0] for s in seeds])      # uint8 [2, H, W]
    H, W = isr.shape[-2:]
    draws = [_golden_sky_draw(z, s, H, W) for s in seeds]
    got = _run_sky(tgt, lab, isr, z['bank'], draws, debug=False, k_host=[d['k'] for d in draws])
    ref = torch.stack([z[f's{s}_sky_out'] for s in seeds])
    check_le('sky mask against the reference', (got - ref).abs().max().item(), 1e-6)
    ndraws = [(int(z[f's{s}_noise_blur']), z[f's{s}_noise_t1'].item(), z[f's{s}_noise_t2'].item(), z[f's{s}_noise_intensity'].item())
              for s in seeds]
    assert sorted(d[0] for d in ndraws) == [0, 1], 'the fixture holds both outcomes of the blur coin'
    fields = torch.stack([z[f's{s}_noise_fields'][:, 0] for s in seeds], 1).contiguous()   # [3, 2, H, W]
    got = ops.isr_noise(tgt.to(isr), tgt.to(ops.isr_noise_params(ndraws)), 'noise+blur', fields=tgt.to(fields)).cpu()
    ref = torch.stack([z[f's{s}_noise_out'] for s in seeds])
    check_le('ISR noise against the reference', (got - ref).abs().max().item(), 1e-6)
