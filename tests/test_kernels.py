"""Kernel-level parity of the HBM-bound kernels against plain torch fp32 (emu on CPU, real lib on GPU)."""
import pytest
import torch
import torch.nn.functional as F

from cmda_amd import ops
from conftest import assert_close, check_le

DT = [(torch.float32, 3e-5), (torch.bfloat16, 1.6e-2)]


@pytest.mark.parametrize('dt,tol', DT)
@pytest.mark.parametrize('C', [32, 64, 128, 160, 320, 1024])
@pytest.mark.parametrize('rows', [37, 9001])
def test_layernorm(tgt, dt, tol, C, rows):
    if rows > 100 and C not in (64, 160):
        pytest.skip('large-row case only for one sub-wave and one full-wave width')
    torch.manual_seed(C)
    x = torch.randn(rows, C).to(dt)
    g, b = torch.randn(C), torch.randn(C)
    dy, dres = torch.randn(rows, C).to(dt), torch.randn(rows, C).to(dt)
    xr = x.float().requires_grad_(True)
    gr, br = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.layer_norm(xr, (C,), gr, br, 1e-6)
    ref.backward(dy.float())
    xd, gd, bd, dyd, dresd = map(tgt.to, (x, g, b, dy, dres))
    y, mean, rstd = ops.layernorm_fwd(xd, gd, bd, 1e-6)
    assert_close(y, ref, tol, name='ln fwd')
    dg, db = torch.zeros(C, device=tgt.device), torch.zeros(C, device=tgt.device)
    dx = ops.layernorm_bwd(dyd, xd, gd, mean, rstd, dg, db, dres=dresd)
    assert_close(dx, xr.grad + dres.float(), tol, name='ln dx')
    assert_close(dg, gr.grad, 2e-5, name='ln dgamma')
    assert_close(db, br.grad, 2e-5, name='ln dbeta')


@pytest.mark.parametrize('dt,tol', DT)
def test_permute_cast_colsum_axpby(tgt, dt, tol):
    torch.manual_seed(0)
    w = torch.randn(6, 5, 3, 3)
    wd = tgt.to(w)
    out = torch.empty(6, 3, 3, 5, dtype=dt, device=tgt.device)
    ops.permute4(wd, out, (6, 5, 3, 3), (0, 2, 3, 1))
    # (bf16: ONE round-to-nearest-even of the fp32 value, i.e. at most 2^-8 of the largest element -- a bound, not a margin)
    assert_close(out, w.permute(0, 2, 3, 1), 4e-3 if dt == torch.bfloat16 else 0, name='permute')
    out = torch.empty(5, 3, 3, 6, dtype=dt, device=tgt.device)
    ops.permute4(wd, out, (6, 5, 3, 3), (1, 2, 3, 0), flipmask=0b1100)
    assert_close(out, w.flip(2, 3).permute(1, 2, 3, 0), 4e-3 if dt == torch.bfloat16 else 0, name='permute+flip')
    g = torch.randn(6, 3, 3, 5)
    acc = tgt.to(w.clone())
    ops.permute4(tgt.to(g), acc, (6, 3, 3, 5), (0, 3, 1, 2), accumulate=True)
    assert_close(acc, w + g.permute(0, 3, 1, 2), 1e-6, name='permute accumulate')
    x = torch.randn(1000, 52).to(dt)
    s = torch.zeros(52, device=tgt.device)
    ops.colsum(tgt.to(x), s, 1000, 52)
    assert_close(s, x.float().sum(0), 1e-5, name='colsum')
    a, b = torch.randn(1003).to(dt), torch.randn(1003).to(dt)
    o = ops.axpby(tgt.to(a), tgt.to(b), 0.5, 0.5)
    assert_close(o, 0.5 * a.float() + 0.5 * b.float(), tol, name='axpby')


@pytest.mark.parametrize('dt,tol', DT)
@pytest.mark.parametrize('L', [24, 256, 280])
def test_softmax(tgt, dt, tol, L):
    torch.manual_seed(L)
    rows = 19
    s = (torch.randn(rows, L) * 3).to(dt)
    sr = s.float().requires_grad_(True)
    ref = torch.softmax(0.125 * sr, -1)
    dp = torch.randn(rows, L).to(dt)
    ref.backward(dp.float())
    p = ops.softmax_fwd_(tgt.to(s.clone()), rows, L, 0.125)
    assert_close(p, ref, tol, name='softmax fwd')
    ds = ops.softmax_bwd_(tgt.to(ref.detach().to(dt)), tgt.to(dp.clone()), rows, L, 0.125)
    assert_close(ds, sr.grad, tol, atol=2e-4 if dt == torch.bfloat16 else 0, name='softmax bwd')


@pytest.mark.parametrize('dt,tol', DT)
@pytest.mark.parametrize('dil,act,shape', [(1, 'gelu', (2, 13, 9, 24)), (1, None, (2, 13, 9, 24)), (6, None, (2, 13, 9, 24)),
                                           (1, 'gelu', (1, 5, 40, 260)), (3, None, (2, 7, 43, 8)), (18, None, (1, 20, 24, 12)),
                                           (12, None, (1, 3, 128, 4))])
def test_dwconv(tgt, dt, tol, dil, act, shape):
    torch.manual_seed(dil)
    B, H, W, C = shape
    x = torch.randn(B, H, W, C).to(dt)
    w, b = torch.randn(C, 1, 3, 3) * 0.3, torch.randn(C)
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    z = F.conv2d(xr, wr, br if act else None, padding=dil, dilation=dil, groups=C)
    ref = F.gelu(z) if act == 'gelu' else z
    dy = torch.randn(B, H, W, C).to(dt)
    ref.backward(dy.float().permute(0, 3, 1, 2))
    xd, wd, bd, dyd = tgt.to(x), tgt.to(w.view(C, 9).t().contiguous()), tgt.to(b) if act else None, tgt.to(dy)  # tap-major [9,C]
    y = ops.dwconv_fwd(xd, wd, bd, B, H, W, C, dil, act)
    assert_close(y, ref.permute(0, 2, 3, 1), tol, name='dw fwd')
    if dil >= 2 and act is None:   # the BatchNorm statistics of the output taken on the way (groups of images: cmda_dwconv3x3_fwd_stats)
        from cmda_amd import _lib as L
        for ipg in (1, B):
            G = B // ipg
            ws = torch.zeros(G * int(L.lib().cmda_bn_ws_floats(C)), device=tgt.device)
            y2 = ops.dwconv_fwd(xd, wd, None, B, H, W, C, dil, None, colstats=(ws, ipg))
            assert torch.equal(y2, y)
            st = ws.view(G, 33, 2, C)[:, :32].sum(1).cpu()
            zr = z.detach().permute(0, 2, 3, 1).reshape(G, ipg * H * W, C)
            assert_close(st[:, 0], zr.sum(1), tol, atol=tol * (ipg * H * W) ** 0.5 * 4, name='dw output column sums')
            assert_close(st[:, 1], (zr * zr).sum(1), tol * 2, name='dw output column sums of squares')
    dz = ops.dwconv_gelu_bwd_prep(xd, wd, bd, dyd, B, H, W, C, dil) if act == 'gelu' else dyd
    dx = ops.dwconv_bwd_data(dz, wd, B, H, W, C, dil)
    assert_close(dx, xr.grad.permute(0, 2, 3, 1), tol * 2, name='dw dx')
    prev = torch.randn(B, H, W, C).to(dt)   # accumulate=True: dx += (the sep-ASPP branches add into one input gradient)
    acc = ops.dwconv_bwd_data(dz, wd, B, H, W, C, dil, out=tgt.to(prev.clone()), accumulate=True)
    assert_close(acc, xr.grad.permute(0, 2, 3, 1) + prev.float(), tol * 3, name='dw dx accumulate')
    dw = torch.zeros(C, 9, device=tgt.device)
    db = torch.zeros(C, device=tgt.device) if act else None
    ops.dwconv_bwd_weight(dz, xd, dw, db, B, H, W, C, dil)
    assert_close(dw, wr.grad.view(C, 9), tol, name='dw dweight')
    if act:
        assert_close(db, br.grad, tol, name='dw dbias')
    if act == 'gelu':   # the fused form of the two calls above (one pass over x / da)
        dw2, db2 = torch.zeros(C, 9, device=tgt.device), torch.zeros(C, device=tgt.device)
        dz2 = ops.dwconv_gelu_bwd_fused(xd, wd, bd, dyd, dw2, db2, B, H, W, C, dil)
        assert_close(dz2, dz, 1e-6 if dt == torch.float32 else 4e-3, name='fused dz')
        assert_close(dw2, wr.grad.view(C, 9), tol, name='fused dweight')
        assert_close(db2, br.grad, tol, name='fused dbias')


@pytest.mark.parametrize('dt,tol', DT)
@pytest.mark.parametrize('IH,IW,OH,OW', [(8, 8, 32, 32), (4, 6, 32, 48), (16, 16, 32, 32), (14, 20, 110, 160), (9, 7, 9, 7)])
def test_bilinear(tgt, dt, tol, IH, IW, OH, OW):
    torch.manual_seed(IH)
    B, C, ld, coff = 2, 8, 24, 12
    x = torch.randn(B, IH, IW, C).to(dt)
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    ref = F.interpolate(xr, size=(OH, OW), mode='bilinear', align_corners=False)
    dy = torch.randn(B, OH, OW, ld).to(dt)
    ref.backward(dy.float()[..., coff:coff + C].permute(0, 3, 1, 2))
    y = torch.zeros(B, OH, OW, ld, dtype=dt, device=tgt.device)
    ops.bilinear_fwd(tgt.to(x), y, B, IH, IW, OH, OW, C, ld, coff)
    assert_close(y[..., coff:coff + C], ref.permute(0, 2, 3, 1), tol if dt == torch.bfloat16 else 2e-6, name='resize fwd')
    assert y[..., :coff].abs().max().item() == 0 and y[..., coff + C:].abs().max().item() == 0
    dx = torch.empty(B, IH, IW, C, dtype=dt, device=tgt.device)
    ops.bilinear_bwd(tgt.to(dy), dx, B, IH, IW, OH, OW, C, ld, coff)
    assert_close(dx, xr.grad.permute(0, 2, 3, 1), tol, name='resize bwd')


@pytest.mark.parametrize('dt,tol', DT)
@pytest.mark.parametrize('relu', [True, False])
def test_batchnorm(tgt, dt, tol, relu):
    torch.manual_seed(3)
    M, C, ld, coff = 600, 36, 48, 8
    x = (torch.randn(M, C) * 2 + 3).to(dt)
    g, b = torch.rand(C) + 0.5, torch.randn(C) * 0.2
    rm, rv = torch.randn(C), torch.rand(C) + 0.5
    bn = torch.nn.BatchNorm1d(C)
    bn.weight.data.copy_(g), bn.bias.data.copy_(b), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    xr = x.float().requires_grad_(True)
    ref = bn(xr)
    ref = F.relu(ref) if relu else ref
    dy = torch.randn(M, ld).to(dt)
    ref.backward(dy.float()[:, coff:coff + C])
    xd, gd, bd, rmd, rvd = map(tgt.to, (x, g, b, rm.clone(), rv.clone()))
    y = torch.zeros(M, ld, dtype=dt, device=tgt.device)
    mean, rstd = ops.bn_train_fwd(xd, gd, bd, y, rmd, rvd, M, C, 1e-5, 0.1, relu, ld, coff)
    assert_close(y[:, coff:coff + C], ref, tol, name='bn fwd')
    assert_close(rmd, bn.running_mean, 1e-5, name='running_mean')
    assert_close(rvd, bn.running_var, 1e-5, name='running_var')
    dg, db = torch.zeros(C, device=tgt.device), torch.zeros(C, device=tgt.device)
    dx = ops.bn_train_bwd(tgt.to(dy), xd, mean, rstd, gd, bd, dg, db, M, C, relu, ld, coff)
    assert_close(dx, xr.grad, tol * 2, name='bn dx')
    assert_close(dg, bn.weight.grad, 1e-4, name='bn dgamma')
    assert_close(db, bn.bias.grad, 1e-4, name='bn dbeta')


@pytest.mark.parametrize('h,w,H,W', [(8, 8, 32, 32), (6, 10, 24, 40), (7, 5, 28, 20), (8, 8, 8, 8), (5, 7, 13, 18), (2, 3, 32, 48), (9, 17, 36, 68),
                                     (12, 20, 24, 40), (10, 9, 30, 27), (32, 40, 128, 160), (11, 13, 66, 65)])   # (tiled backward: factors 2 / 3 / 4 / 5-6, several tiles)
@pytest.mark.parametrize('use_weight', [True, False])
def test_ce_upsample(tgt, h, w, H, W, use_weight):
    torch.manual_seed(h * 3 + w)
    B, nc = 2, (19 if (h + w) % 3 else 7)   # (19: the unrolled instance of the tiled backward; 7: its run-time class count)
    logits = torch.randn(B, h, w, nc) * 2
    label = torch.randint(0, nc, (B, H, W))
    label[torch.rand(B, H, W) < 0.1] = 255
    weight = torch.rand(B, H, W) if use_weight else None
    lr = logits.permute(0, 3, 1, 2).clone().requires_grad_(True)
    up = F.interpolate(lr, size=(H, W), mode='bilinear', align_corners=False)
    loss_px = F.cross_entropy(up, label, reduction='none', ignore_index=255)
    if use_weight:
        loss_px = loss_px * weight
    loss = loss_px.mean()
    (loss * 0.7).backward()
    acc_ref = (up.argmax(1) == label).float().sum()
    acc, lse = ops.ce_upsample_fwd(tgt.to(logits), tgt.to(label), tgt.to(weight), H, W)
    n = B * H * W
    assert_close(acc[0] / n, loss, 2e-6, name='ce loss')
    assert acc[1].item() == acc_ref.item()
    gs = tgt.to(torch.tensor([0.7]))
    dl = ops.ce_upsample_bwd(tgt.to(logits), tgt.to(label), tgt.to(weight), lse, gs, 1.0 / n, H, W)
    assert_close(dl, lr.grad.permute(0, 2, 3, 1), 2e-5, name='ce dlogits')


def test_pseudo_label(tgt):
    torch.manual_seed(5)
    B, h, w, H, W, nc = 2, 8, 12, 32, 48, 19
    logits = torch.randn(B, h, w, nc) * 4
    up = F.interpolate(logits.permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=False)
    prob_ref, lab_ref = torch.softmax(up, 1).max(1)
    lab, prob, cnt = ops.pseudo_label(tgt.to(logits), H, W, 0.968)
    top2 = up.topk(2, 1).values
    near_tie = (top2[:, 0] - top2[:, 1]) < 1e-5
    assert bool(((lab.cpu() == lab_ref) | near_tie).all())
    assert_close(prob, prob_ref, 1e-5, name='pseudo prob')
    assert abs(cnt.item() - int((prob_ref >= 0.968).sum())) <= 2
    wgt = ops.pseudo_weight(cnt, B, H, W, top=3, bottom=5)
    exp = torch.full((B, H, W), cnt.item() / (B * H * W))
    exp[:, :3] = 0
    exp[:, H - 5:] = 0
    assert_close(wgt, exp, 1e-7, name='pseudo weight')


def test_classmix_ema_adamw(tgt):
    torch.manual_seed(7)
    B, C, H, W = 2, 3, 8, 10
    src, tg = torch.randn(B, C, H, W), torch.randn(B, C, H, W)
    lab = torch.randint(0, 5, (B, H, W))
    classes = torch.tensor([[1, 3, -1], [0, 2, 4]])
    mask = torch.stack([(lab[i][None] == classes[i][classes[i] >= 0][:, None, None]).sum(0) for i in range(B)]).float()
    out = ops.class_mix(tgt.to(src), tgt.to(tg), tgt.to(lab), tgt.to(classes))
    assert_close(out, mask[:, None] * src + (1 - mask[:, None]) * tg, 0, name='classmix')
    plab = torch.randint(0, 19, (B, H, W))
    ol = ops.class_mix_label(tgt.to(lab), tgt.to(plab), tgt.to(lab), tgt.to(classes))
    assert torch.equal(ol.cpu(), (mask.long() * lab + (1 - mask.long()) * plab))
    p, e = torch.randn(1001), torch.randn(1001)
    ed = tgt.to(e.clone())
    ops.ema_update(ed, tgt.to(p), 0.9)
    assert_close(ed, 0.9 * e + 0.1 * p, 1e-6, name='ema')
    prm = torch.nn.Parameter(torch.randn(777))
    opt = torch.optim.AdamW([prm], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    pd = tgt.to(prm.data.clone())
    m, v = torch.zeros(777, device=tgt.device), torch.zeros(777, device=tgt.device)
    pb = torch.empty(777, dtype=torch.bfloat16, device=tgt.device)
    for step in (1, 2, 3):
        gr = torch.randn(777)
        prm.grad = gr.clone()
        opt.step()
        ops.adamw_step(pd, tgt.to(gr), m, v, 1e-2, 0.9, 0.999, 1e-8, 0.01, step, p_bf16=pb)
    assert_close(pd, prm.data, 2e-6, name='adamw')
    assert_close(pb, prm.data, 4e-3, name='adamw bf16 copy')   # one rounding of the updated fp32 master: <= 2^-8 of the largest element


def _gold(name):
    import os
    import numpy as np
    here = os.path.dirname(os.path.abspath(__file__))
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(here, 'golden', name + '.npz')).items()}


def test_isr_golden(tgt):
    """On-device Image Content-Extractor vs the reference's get_image_change_from_pil outputs (tests/golden/isr.npz)."""
    from oracle import uda as ouda
    g = _gold('isr')
    img_u8 = g['img']  # [H,W,3] uint8
    # build the normalised image whose denorm*255 truncates back to img_u8 (as the step does with the mixed image)
    mean = torch.tensor(ouda.IMG_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(ouda.IMG_STD).view(1, 3, 1, 1)
    x = ((img_u8.permute(2, 0, 1)[None].float() + 0.5) - mean) / std
    gray = ops.isr_gray(tgt.to(x.contiguous()))
    assert torch.equal(gray.cpu()[0], g['gray'])
    params = {'dsec': dict(val_range=[0.01, 1.01], threshold=0.005, clip_range=0.1, shift_pixel=1),
              'dz': dict(val_range=[1, 100], threshold=0.01, clip_range=0.1, shift_pixel=3)}
    for pn, p in params.items():
        for d in ('rightdown', 'rightup', 'leftdown', 'leftup', 'all'):
            out = ops.isr_from_gray(gray, shift_direction=d, **p)
            assert_close(out[0, 0:1], g[f'{pn}_{d}'], 2e-6, atol=2e-7, name=f'isr {pn} {d}')
            assert torch.equal(out[0, 0], out[0, 2])


def test_voxel_golden(tgt):
    g = _gold('voxel')
    for bins in (1, 5):
        vg = ops.events_to_voxel_grid(*[tgt.to(g[f'{k}{bins}']) for k in 'txyp'], bins, 48, 64)
        assert_close(vg, g[f'vg{bins}'], 2e-6, atol=1e-6, name='voxel grid')
        nrm = ops.events_norm(tgt.to(g[f'vg{bins}']), (5000 / 500000) * 1.5 * 100)
        assert_close(nrm, g[f'norm{bins}'], 1e-5, name='events_norm')


def test_strong_augmentation(tgt):
    """per-sample colour-jitter parameters and the (ky from H, kx from W) blur of dacs_transforms.py:64-98, plus the device-side
    on/off gates a captured launch sequence relies on"""
    from oracle import uda as ouda
    torch.manual_seed(9)
    img = torch.randn(2, 3, 40, 56)
    per_sample = [([2, 0, 3, 1], 1.1, 0.9, 1.15, -0.07), ([1, 3, 0, 2], 0.85, 1.2, 0.8, 0.11)]
    ref = torch.cat([ouda.color_jitter(img[i:i + 1], *per_sample[i]) for i in range(2)])
    prm = tgt.to(ops.jitter_params(per_sample))
    on, off = tgt.to(torch.ones(1, dtype=torch.int32)), tgt.to(torch.zeros(1, dtype=torch.int32))
    out = ops.color_jitter_(tgt.to(img.clone()), prm, on)
    assert_close(out, ref, 1e-4, atol=2e-4, name='color jitter', outlier_frac=1e-3, outlier_rtol=2.0)
    assert torch.equal(ops.color_jitter_(tgt.to(img.clone()), prm, off).cpu(), img), 'gate off must leave the image untouched'
    ky, kx = ouda.blur_kernel_size(40), ouda.blur_kernel_size(56)
    assert (ky, kx) == (ops.blur_kernel_size(40), ops.blur_kernel_size(56)) and ky != kx
    refb = ouda.gaussian_blur_hw(img, ky, kx, 0.8)
    tx, ty = tgt.to(ops.gaussian_taps(kx, 0.8)), tgt.to(ops.gaussian_taps(ky, 0.8))
    outb = ops.gaussian_blur_(tgt.to(img.clone()), tx, ty, on)
    assert_close(outb, refb, 1e-5, atol=1e-6, name='gaussian blur')
    assert torch.equal(ops.gaussian_blur_(tgt.to(img.clone()), tx, ty, off).cpu(), img), 'gate off must leave the image untouched'


def _attention_ref(q, kv, B, N, Nk, heads, C, scale):
    hd = C // heads
    qf = q.view(B, N, heads, hd).permute(0, 2, 1, 3)
    k = kv[:, :C].reshape(B, Nk, heads, hd).permute(0, 2, 1, 3)
    v = kv[:, C:].reshape(B, Nk, heads, hd).permute(0, 2, 1, 3)
    a = (qf @ k.transpose(-1, -2) * scale).softmax(-1)  # mix_transformer.py:97-99
    return (a @ v).permute(0, 2, 1, 3).reshape(B * N, C)


@pytest.mark.parametrize('B,N,Nk,heads', [(1, 64, 256, 1), (2, 200, 256, 2), (1, 70, 37, 1), (1, 300, 130, 5), (2, 520, 256, 1),
                                          (16, 4100, 256, 2), (64, 130, 20, 8)])
def test_fused_attention(tgt, B, N, Nk, heads):
    if B * N > 20000 and tgt.device.type != 'cuda':   # (the 128-queries-per-block launch runs everywhere at (64, 130, 20, 8): 1024 blocks)
        pytest.skip('65 600 queries x 256 keys: GPU only (emulator run time)')
    """fused softmax(q k^T) v and its backward (probabilities recomputed in LDS) against autograd on the same bf16 inputs"""
    torch.manual_seed(N + Nk)
    C, scale = heads * 64, 0.125
    q, kv, do = torch.randn(B * N, C).bfloat16(), torch.randn(B * Nk, 2 * C).bfloat16(), torch.randn(B * N, C).bfloat16()
    qr, kvr = q.float().requires_grad_(True), kv.float().requires_grad_(True)
    ref = _attention_ref(qr, kvr, B, N, Nk, heads, C, scale)
    ref.backward(do.float())
    qd, kvd, dod = tgt.to(q), tgt.to(kv), tgt.to(do)
    assert ops.attention_fused_ok(qd, Nk, heads, C)
    o = ops.attention_fused_fwd(qd, kvd, B, N, Nk, heads, C, scale)
    assert_close(o, ref.detach(), 1.6e-2, name='attention o')
    dkv = torch.zeros(B * Nk, 2 * C, device=tgt.device)
    dq = ops.attention_fused_bwd(qd, kvd, dod, dkv, B, N, Nk, heads, C, scale)   # accumulating form: fp32 workspace + atomics
    assert_close(dq, qr.grad, 2e-2, name='attention dq')
    assert_close(dkv[:, :C], kvr.grad[:, :C], 2e-2, name='attention dk')   # (dK and dV each against its own maximum)
    assert_close(dkv[:, C:], kvr.grad[:, C:], 2e-2, name='attention dv')
    assert ops.attention_bwd_direct(B, N, Nk, heads) == (N <= 1024)
    if ops.attention_bwd_direct(B, N, Nk, heads):   # few queries: one block per key slice, dK | dV stored straight as bf16
        dkv16 = torch.full((B * Nk, 2 * C), float('nan'), dtype=torch.bfloat16, device=tgt.device)
        dq2 = ops.attention_fused_bwd(qd, kvd, dod, None, B, N, Nk, heads, C, scale, dkv16=dkv16)
        assert_close(dq2, qr.grad, 2e-2, name='attention dq (direct)')
        assert_close(dkv16[:, :C], kvr.grad[:, :C], 2e-2, name='attention dk (direct)')
        assert_close(dkv16[:, C:], kvr.grad[:, C:], 2e-2, name='attention dv (direct)')


@pytest.mark.parametrize('B,N,Nk,heads', [(1, 64, 256, 1), (2, 200, 256, 2), (1, 70, 37, 1), (1, 300, 130, 5), (2, 1100, 256, 1)])
def test_fused_attention_split_bf16(tgt, B, N, Nk, heads):
    """the split-bf16 instances of the fused attention kernels (fp32 storage, three bf16 MFMAs per product: the tolerance-meeting
    mode's mix_transformer.py:97-101): forward, dq, dK | dV in the accumulating and the direct form, against fp32 autograd -- the
    error of ~16 mantissa bits per product, two orders below the bf16 kernels'"""
    if B * N > 1500 and tgt.device.type != 'cuda':
        pytest.skip('query counts beyond the direct mode: GPU only (emulator run time)')
    torch.manual_seed(N + Nk)
    C, scale = heads * 64, 0.125
    q, kv, do = torch.randn(B * N, C), torch.randn(B * Nk, 2 * C), torch.randn(B * N, C)
    qr, kvr = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    ref = _attention_ref(qr, kvr, B, N, Nk, heads, C, scale)
    ref.backward(do)
    qd, kvd, dod = tgt.to(q), tgt.to(kv), tgt.to(do)
    assert ops.attention_fused_ok(qd, Nk, heads, C, x3=True) and not ops.attention_fused_ok(qd, Nk, heads, C)
    o = ops.attention_fused_fwd(qd, kvd, B, N, Nk, heads, C, scale)
    assert o.dtype == torch.float32
    assert_close(o, ref.detach(), 1e-4, name='split-bf16 attention o')
    dkv = torch.zeros(B * Nk, 2 * C, device=tgt.device)
    dq = ops.attention_fused_bwd(qd, kvd, dod, dkv, B, N, Nk, heads, C, scale)   # accumulating form: fp32 atomics
    assert_close(dq, qr.grad, 2e-4, name='split-bf16 attention dq')
    assert_close(dkv[:, :C], kvr.grad[:, :C], 2e-4, name='split-bf16 attention dk')
    assert_close(dkv[:, C:], kvr.grad[:, C:], 2e-4, name='split-bf16 attention dv')
    if ops.attention_bwd_direct(B, N, Nk, heads):   # few queries: one block per key slice stores dK | dV (fp32)
        dkv2 = torch.full((B * Nk, 2 * C), float('nan'), device=tgt.device)
        dq2 = ops.attention_fused_bwd(qd, kvd, dod, None, B, N, Nk, heads, C, scale, dkv16=dkv2)
        assert_close(dq2, qr.grad, 2e-4, name='split-bf16 attention dq (direct)')
        assert_close(dkv2[:, :C], kvr.grad[:, :C], 2e-4, name='split-bf16 attention dk (direct)')
        assert_close(dkv2[:, C:], kvr.grad[:, C:], 2e-4, name='split-bf16 attention dv (direct)')
    # through the block-level composite: runtime.gemm_x3 routes fp32 storage to these kernels; same result as the unfused products
    from cmda_amd import nn as K
    import cmda_amd.runtime as rt
    rt.set_compute_dtype(torch.float32)
    rt.set_gemm_x3(True)
    try:
        o1, P1 = K.attention_fwd(qd, kvd, B, N, Nk, heads, C, scale)
        assert P1 is None
        dq1, dkv1 = K.attention_bwd(dod, qd, kvd, None, B, N, Nk, heads, C, scale)
        ops.ATTN_X3_OFF = True
        o2, P2 = K.attention_fwd(qd, kvd, B, N, Nk, heads, C, scale)
        assert P2 is not None
        dq2, dkv2 = K.attention_bwd(dod, qd, kvd, P2, B, N, Nk, heads, C, scale)
    finally:
        ops.ATTN_X3_OFF = False
        rt.set_gemm_x3(False)
    assert_close(o1, o2, 1e-4, name='fused vs unfused split-bf16 attention')
    assert_close(dq1, dq2, 2e-4, name='fused vs unfused split-bf16 dq')
    assert_close(dkv1[:, :C], dkv2[:, :C], 2e-4, name='fused vs unfused split-bf16 dk')
    assert_close(dkv1[:, C:], dkv2[:, C:], 2e-4, name='fused vs unfused split-bf16 dv')


@pytest.mark.parametrize('B,N,Nk,heads', [(1, 1120, 280, 2), (2, 280, 260, 5), (1, 70, 320, 8), (1, 300, 257, 1)])
def test_fused_attention_eval_keys(tgt, B, N, Nk, heads):
    """inference on 440 x 640 frames leaves 260 / 280 keys after the spatial reduction (encoder_decoder.py:897-936, mix_transformer.py
    sr_ratios): the forward-only instance of the fused kernel holds up to 320 keys; the training kernels stay at 256"""
    torch.manual_seed(N + Nk)
    C, scale = heads * 64, 0.125
    q, kv = torch.randn(B * N, C).bfloat16(), torch.randn(B * Nk, 2 * C).bfloat16()
    ref = _attention_ref(q.float(), kv.float(), B, N, Nk, heads, C, scale)
    qd, kvd = tgt.to(q), tgt.to(kv)
    assert ops.attention_fused_ok(qd, Nk, heads, C, need_grad=False) and not ops.attention_fused_ok(qd, Nk, heads, C)
    o = ops.attention_fused_fwd(qd, kvd, B, N, Nk, heads, C, scale)
    assert_close(o, ref, 1.6e-2, name='attention o (eval keys)')
    # and through the block: save=False (no backward to follow) takes the fused kernel, save=True the materialised path; same output
    from cmda_amd import nn as K
    import cmda_amd.runtime as rt
    rt.set_compute_dtype(torch.bfloat16)
    try:
        o1, P1 = K.attention_fwd(qd, kvd, B, N, Nk, heads, C, scale, need_grad=False)
        o2, P2 = K.attention_fwd(qd, kvd, B, N, Nk, heads, C, scale, need_grad=True)
    finally:
        rt.set_compute_dtype(torch.float32)
    assert P1 is None and P2 is not None
    assert_close(o1, o2.float(), 4e-2, name='fused vs materialised')   # (bf16 outputs one ulp apart: 7.8e-3 of range measured)


# ------------------------------------------------------------------ round-3 entry points, each against torch
@pytest.mark.parametrize('C,rows', [(64, 300), (320, 130), (512, 33), (128, 1000)])
def test_layernorm_fp32_stream_bf16_operands(tgt, C, rows):
    """cmda_layernorm_fwd2 / bwd2: the fp32 residual stream in, the bf16 GEMM operand out; backward: bf16 gradients in and out, the
    statistics recomputed from the fp32 input (mix_transformer.py:141-146 with x kept in fp32)"""
    torch.manual_seed(C + rows)
    x = torch.randn(rows, C) * 3 + 1
    g, b = torch.randn(C), torch.randn(C)
    dy, dres = torch.randn(rows, C).bfloat16(), torch.randn(rows, C).bfloat16()
    xr = x.clone().requires_grad_(True)
    gr, br = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.layer_norm(xr, (C,), gr, br, 1e-6)
    ref.backward(dy.float())
    xd, gd, bd, dyd, dresd = map(tgt.to, (x, g, b, dy, dres))
    y, mean, rstd = ops.layernorm_fwd(xd, gd, bd, 1e-6, out_dtype=torch.bfloat16)
    assert y.dtype == torch.bfloat16
    assert_close(y, ref, 8e-3, name='ln fwd fp32 -> bf16')            # one rounding of the exact fp32 result
    assert_close(mean, x.mean(1), 1e-5, name='ln mean')
    dg, db = torch.zeros(C, device=tgt.device), torch.zeros(C, device=tgt.device)
    sc = torch.rand(4)
    rps = (rows + 3) // 4
    dx, dxs = ops.layernorm_bwd(dyd, xd, gd, mean, rstd, dg, db, dres=dresd, out_scale=tgt.to(sc), rows_per_scale=rps)
    assert dx.dtype == torch.bfloat16
    want = xr.grad + dres.float()
    assert_close(dx, want, 1.6e-2, name='ln dx (bf16 out)')
    assert_close(dxs, want * sc[torch.arange(rows) // rps, None], 1.6e-2, name='ln dx scaled')
    assert_close(dg, gr.grad, 2e-5, name='ln dgamma')
    assert_close(db, br.grad, 2e-5, name='ln dbeta')


@pytest.mark.parametrize('M,N,K', [(300, 64, 64), (130, 320, 1280), (1000, 128, 512)])
def test_gemm_fp32_residual_epilogue(tgt, M, N, K):
    """x1 = x + drop_path(proj(o)) with x and x1 in fp32 and the GEMM operands in bf16 (cmda_gemm_params_t.res_f32): the residual is
    added in fp32 in the epilogue, per-sample DropPath scale on the GEMM term only"""
    torch.manual_seed(M)
    a, w, bias = torch.randn(M, K).bfloat16(), (torch.randn(N, K) * 0.05).bfloat16(), torch.randn(N)
    res = torch.randn(M, N) * 50          # large against the GEMM term: a bf16 residual add would lose ~0.2 absolute here
    sc = torch.tensor([0.0, 1.25, 1.25, 0.0])
    rps = (M + 3) // 4
    ref = res + (a.float() @ w.float().t() + bias) * sc[torch.arange(M) // rps, None]
    out = torch.empty(M, N, dtype=torch.float32, device=tgt.device)
    ad, wd = tgt.to(a), tgt.to(w)
    ops.gemm(ops.plain_view(ad, M, K), ops.plain_view(wd, N, K), out, M, N, K, dtype=1, bias=tgt.to(bias), res=tgt.to(res),
             rowscale=tgt.to(sc), rows_per_scale=rps)
    err = (out.cpu() - ref).abs().max().item()
    check_le('fp32 residual epilogue: max abs err', err, 2e-3, strict=True)


@pytest.mark.parametrize('dt,tol', [(torch.bfloat16, 2e-3), (torch.float32, 2e-5)])
def test_conv_co1(tgt, dt, tol):
    """the generator's last layer, Conv2d(64, 1, 7, padding 3 reflect) + tanh (cyclegan_model.py:372-374), as a dot-product stencil
    (bf16: v_dot2; fp32 storage -- both parity modes --: plain FMAs over channel chunks)"""
    torch.manual_seed(3)
    B, H, W, C, K = 2, 19, 23, 64, 7
    x = torch.randn(B, C, H, W).to(dt)
    w = (torch.randn(1, C, K, K) * 0.05).to(dt)
    bias = torch.randn(1)
    for reflect in (True, False):
        xp = F.pad(x.float(), (3, 3, 3, 3), mode='reflect') if reflect else F.pad(x.float(), (3, 3, 3, 3))
        ref = torch.tanh(F.conv2d(xp, w.float(), bias))[:, 0]
        xd = tgt.to(x.permute(0, 2, 3, 1).reshape(-1, C).contiguous())
        wd = tgt.to(w.permute(0, 2, 3, 1).reshape(-1).contiguous())
        assert ops.conv_co1_ok(xd, C, K, 3)
        out = ops.conv_co1(xd, wd, tgt.to(bias), B, H, W, C, K, 3, reflect, 'tanh')
        assert_close(out, ref, tol, name=f'conv_co1 reflect={reflect}')


def test_rows_fill_cast_pad_nchw_pad(tgt):
    torch.manual_seed(4)
    bias = torch.randn(20)
    out = ops.rows_fill(torch.full((37, 20), float('nan'), device=tgt.device), tgt.to(bias))
    assert torch.equal(out.cpu(), bias.expand(37, 20))
    out = ops.rows_fill(torch.full((5, 8), float('nan'), device=tgt.device), None)
    assert torch.equal(out.cpu(), torch.zeros(5, 8))
    src = torch.randn(33, 27)
    for dt in (torch.float32, torch.bfloat16):
        dst = ops.cast_pad_cols(tgt.to(src), 32, dt)
        assert dst.shape == (33, 32) and dst.dtype == dt
        assert torch.equal(dst[:, :27].cpu().float(), src.to(dt).float()) and not dst[:, 27:].cpu().float().abs().any()
    img = torch.randn(2, 3, 7, 9)
    for dt in (torch.float32, torch.bfloat16):
        dst = torch.full((2 * 63, 8), float('nan'), dtype=dt, device=tgt.device)
        ops.nchw_to_nhwc_pad(tgt.to(img), dst, 2, 3, 63, 8)
        want = torch.zeros(2, 7, 9, 8)
        want[..., :3] = img.permute(0, 2, 3, 1)
        assert torch.equal(dst.cpu().float(), want.view(-1, 8).to(dt).float())


# ------------------------------------------------------------------ BatchNorm family (csrc/batchnorm.hip) against float64
# The checker is float64 torch written out here, on the stored inputs (bf16 values widened): mean, biased variance, eps inside the
# square root, unbiased variance for running_var, the momentum blend applied group by group in `order`.
_BN_ORDER = {1: None, 2: (1, 0), 3: (2, 0, 1), 4: (2, 0, 3, 1), 8: (5, 2, 7, 0, 3, 6, 1, 4)}


def _bn_rows_per_block(rows_total, C):
    """rows_per_block / rows_per_block_apply of batchnorm.hip restated: halve from 512 / 256 while the grid stays under 1024 / 2048
    blocks, down to 32 / 16 (rows_total = rows per group x groups, gx = channel blocks of 256)"""
    gx = (C // 4 + 63) // 64
    red, app = 512, 256
    while red > 32 and -(-rows_total // red) * gx < 1024:
        red >>= 1
    while app > 16 and -(-rows_total // app) * gx < 2048:
        app >>= 1
    return red, app


def _bn_inputs(M, C, G, dt, seed):
    """x ~ N(3 + 7 g, 2^2) in group g (the inputs of test_batchnorm; the group means lie 3.5 standard deviations apart, so another
    group's mean / rstd is visibly wrong), gamma in [0.5, 1.5], beta ~ 0.2 N(0, 1)"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(G, M, C, generator=gen) * 2 + 3
    x += 7.0 * torch.arange(G, dtype=torch.float32).view(G, 1, 1)
    return x.to(dt), torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.2, gen


def _bn_ref64(x, g, b, eps):
    """x [G, M, C] stored values -> float64 mean, biased variance, rstd [G, C], xhat and the pre-activation [G, M, C]"""
    x64 = x.double()
    mean = x64.mean(1)
    var = ((x64 - mean[:, None]) ** 2).mean(1)
    rstd = (var + eps).rsqrt()
    xhat = x64.sub_(mean[:, None]).mul_(rstd[:, None])
    return mean, var, rstd, xhat, xhat * g.double() + b.double()


def _bn_train_case(tgt, dt, tol, relu, M, C, G, ld, coff, seed):
    eps, mom = 1e-5, 0.1
    order = _BN_ORDER[G]
    x, g, b, gen = _bn_inputs(M, C, G, dt, seed)
    rm0, rv0 = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    dg0, db0 = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    mean, var, rstd, xhat, pre = _bn_ref64(x, g, b, eps)
    shift = x[:, 0].double()
    dy = torch.randn(G * M, ld, generator=gen).to(dt)
    dys = dy.view(G, M, ld)[:, :, coff:coff + C]
    band = None
    if relu:
        # The gradient of an element whose pre-activation is within rounding of zero is arbitrary, and it is the element's WHOLE
        # gradient.  Exactly the elements whose float64 pre-activation lies within 1e-4 of zero are left out of the dx comparison (at
        # most 1e-3 of a case, asserted on the reference alone); everything else is compared with no allowance.  dy is zero on those
        # elements, so a mask the kernel's own statistics (1e-6 off) flip there moves neither dgamma / dbeta nor the dx of the other
        # elements: those keep their plain bounds at every size (at 4 x 32768 x 1024 a handful of flips per case is expected, each
        # worth |dy| ~ 1 against a dbeta bound of 0.1).
        band = pre.abs() < 1e-4
        check_le('bn relu: share of elements within 1e-4 of the mask edge', band.double().mean().item(), 1e-3)
        dys.masked_fill_(band, 0)
    dy64 = dys.double()
    if relu:
        dy64 = dy64 * (pre > 0)
    yref = pre.clamp_(min=0) if relu else pre
    s1, s2 = dy64.sum(1), (dy64 * xhat).sum(1)
    dxref = (dy64 - s1[:, None] / M - xhat.mul_(s2[:, None] / M)).mul_((g.double() * rstd)[:, None])
    # running statistics: the float64 recurrence, group after group in `order`.  M = 1: bn_finalize_kernel skips the unbiased factor
    # M / (M - 1) (torch raises there; the contract of the kernel is running_var <- blend with the biased variance, 0)
    rm, rv = rm0.double(), rv0.double()
    for i in (order or range(G)):
        rm = (1 - mom) * rm + mom * mean[i]
        rv = (1 - mom) * rv + mom * (var[i] * M / (M - 1) if M > 1 else var[i])
    xd, gd, bd, rmd, rvd = map(tgt.to, (x.view(G * M, C), g, b, rm0.clone(), rv0.clone()))
    y = torch.zeros(G * M, ld, dtype=dt, device=tgt.device)
    mean_k, rstd_k = ops.bn_train_fwd(xd, gd, bd, y, rmd, rvd, M, C, eps, mom, relu, ld, coff, groups=G, order=order)
    assert_close(y[:, coff:coff + C], yref.view(G * M, C), tol, name='bn fwd')
    assert not y[:, :coff].any().item() and not y[:, coff + C:].any().item(), 'columns outside the slice were written'
    assert_close(mean_k, mean, 1e-5, name='bn saved mean')
    if M > 1:
        # 1e-5 (the project's bound for the statistics of well-conditioned input, relative here to each channel's own rstd) plus the
        # channel's conditioning term: the variance is taken in one pass around row 0 of the group, its relative error is at most
        # K 2^-24 kappa (test_batchnorm_conditioning) and rstd's half that.  kappa reaches ~20 here (row 0 up to 4.4 sigma off its
        # channel's mean): a plain 1e-5 of max rstd was within 1.5x at 4 x 32768 x 1024 on an MI355X (6.7e-6), and the conditioning
        # term alone, measured at 4096 rows, within 1.2x at 600000 rows on the emulator (longer fp32 sums: 8.6 x 2^-24 kappa).
        # Wrong statistics (another group's, a lost row block) are off by orders of magnitude more.
        kappa = 1 + (mean - shift) ** 2 / var
        bound = 1e-5 + _BN_COND_K / 2 * 2.0 ** -24 * kappa
        check_le('bn saved rstd: relative error / (1e-5 + K/2 2^-24 kappa)', ((rstd_k.double().cpu() - rstd).abs() / rstd / bound).max().item(), 1.0)
    else:
        assert_close(rstd_k, rstd, 1e-5, name='bn saved rstd')   # (one row: variance 0 exactly, rstd = eps^-1/2)
    assert_close(rmd, rm, 1e-5, name='running_mean')
    assert_close(rvd, rv, 1e-5, name='running_var')
    dg, db = tgt.to(dg0.clone()), tgt.to(db0.clone())   # (the kernels add into dgamma / dbeta)
    dx = ops.bn_train_bwd(tgt.to(dy), xd, mean_k, rstd_k, gd, bd, dg, db, M, C, relu, ld, coff, groups=G)
    dx, dxref = dx.float().cpu().view(G, M, C), dxref
    if relu:
        dx, dxref = dx[~band], dxref[~band]
    if M > 2:
        assert_close(dx, dxref, tol, name='bn dx')
    else:
        # one row: dx = 0; two rows: xhat = +-1 and dx cancels to O(eps / var) of its terms (max |dx| 2e-4 here), so the fp32 rounding
        # of the terms is not small against max |dx|.  The bound is taken relative to the terms' size max |gamma rstd dy| -- what
        # max |dx| is in every other case
        assert_close(dx, dxref, 0, atol=tol * ((g.double() * rstd).abs().max() * dy64.abs().max()).item(), name='bn dx (M <= 2)')
    assert_close(dg, dg0.double() + s2.sum(0), 1e-4, name='bn dgamma')
    assert_close(db, db0.double() + s1.sum(0), 1e-4, name='bn dbeta')


# (rows per group M, C, groups).  Edges: M = 1 / 2, fewer rows than the 4-row unroll x 4 row lanes, ragged tails, C over several
# 256-channel blocks and not a multiple of 256.  Then one case per rows_per_block pair (reduce / apply), recomputed from the heuristics
# with rows = M x groups and gx = 1 (C <= 256): every one has more than 32 row blocks PER GROUP, so the 32 workspace slots wrap
#   (600000, 4, 1): ceil(600000 / 512) = 1172 >= 1024 -> 512;  ceil(600000 / 256) = 2344 >= 2048 -> 256      1172 blocks per group
#   (37500, 4, 8):  300000 / 512 = 586, / 256 = 1172 -> 256;   / 256 = 1172, / 128 = 2344 -> 128              147 blocks per group
#   (150000, 4, 1): 293, 586, / 128 = 1172 -> 128;             586, 1172, / 64 = 2344 -> 64                   1172 blocks per group
#   (35000, 4, 2):  70000: 137, 274, 547, / 64 = 1094 -> 64;   274, 547, 1094, / 32 = 2188 -> 32              547 blocks per group
#   (20000, 256, 1): 40, 79, 157, 313 -> floor 32;             79, 157, 313, 625 -> floor 16                  625 blocks per group
# (the head shapes of test_batchnorm_head_shapes: 4 x 32768 rows, C = 256 -> 128 / 64; C = 1024, gx = 4 -> 512 / 256)
_BN_EDGES = [(1, 8, 1), (2, 8, 1), (5, 4, 1), (37, 260, 1), (4099, 260, 1), (1000, 516, 3), (515, 1028, 2)]
_BN_RPB = {(600000, 4, 1): (512, 256), (37500, 4, 8): (256, 128), (150000, 4, 1): (128, 64), (35000, 4, 2): (64, 32),
           (20000, 256, 1): (32, 16)}


@pytest.mark.parametrize('dt,tol', DT)
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('M,C,G', _BN_EDGES + list(_BN_RPB))
def test_batchnorm_shapes(tgt, dt, tol, relu, M, C, G):
    """cmda_bn_train_fwd + cmda_bn_train_bwd against float64 at the shapes where the kernels' indexing can go wrong: y inside its
    column slice and zeros outside, saved mean / rstd per group, the running statistics after a grouped call (from non-trivial
    starting values, groups applied in `order`), dx, dgamma / dbeta accumulated onto non-zero starting values.
    M = 1 follows bn_finalize_kernel: the unbiased factor is skipped."""
    if (M, C, G) in _BN_RPB:
        assert _bn_rows_per_block(M * G, C) == _BN_RPB[(M, C, G)] and M > 32 * _BN_RPB[(M, C, G)][0]
    _bn_train_case(tgt, dt, tol, relu, M, C, G, ld=C + 12, coff=8, seed=M + C + G)


@pytest.mark.parametrize('dt,tol', DT)
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('C,ld,coff', [(256, 1024, 0), (256, 1024, 256), (256, 1024, 768), (1024, 1024, 0)])
@pytest.mark.parametrize('rows', [2048, 32768])
def test_batchnorm_head_shapes(tgt, dt, tol, relu, C, ld, coff, rows):
    """the decode head's calls: a 256-channel slice of the 1024-channel ASPP concat buffer (ldy = lddy = 1024) and the depthwise
    branch's 1024 channels, four groups (image / events / fusion / ISR features through the shared decoder) with their running
    statistics applied in the order (2, 0, 3, 1); 2 x 128 x 128 rows per group as in training, 2048 on the emulator too"""
    if rows > 2048 and tgt.device.type != 'cuda':
        pytest.skip('the full 2 x 128 x 128 rows per group: GPU only (emulator run time)')
    if rows == 32768:
        assert _bn_rows_per_block(4 * rows, C) == ((128, 64) if C == 256 else (512, 256))
    _bn_train_case(tgt, dt, tol, relu, rows, C, 4, ld=ld, coff=coff, seed=C + coff)


_F32, _BF16 = torch.float32, torch.bfloat16
# (groups, rows per group, C, affine, relu): every value of groups 1 / 3 / 8, rows 515 / 4096, C 72 / 256, InstanceNorm's
# gamma = 1, beta = 0 (cyclegan._inorm) and a general gamma / beta, ReLU on and off
_BN2_CASES = [(1, 515, 72, 'unit', True), (3, 4096, 72, 'general', False), (8, 515, 256, 'general', True),
              (3, 515, 256, 'unit', False), (8, 4096, 256, 'unit', True), (1, 4096, 72, 'general', True)]


@pytest.mark.parametrize('G,M,C,affine,relu', _BN2_CASES)
@pytest.mark.parametrize('use_y2', [False, True], ids=['noy2', 'y2'])
@pytest.mark.parametrize('use_res', [False, True], ids=['nores', 'res32'])
@pytest.mark.parametrize('ydt', [_F32, _BF16], ids=['y32', 'y16'])
@pytest.mark.parametrize('xdt', [_F32, _BF16], ids=['x32', 'x16'])
def test_bn_train_fwd2(tgt, xdt, ydt, use_res, use_y2, G, M, C, affine, relu):
    """cmda_bn_train_fwd2 (the generator's InstanceNorm: one group per sample) against float64: x and y of independent storage types,
    the fp32 residual added AFTER the ReLU, the bf16 copy y2 with pitch C whatever ldy is, y a column slice (ldy > C, coff > 0)"""
    ld, coff = C + 24, 16
    x, g, b, gen = _bn_inputs(M, C, G, xdt, G * M + C)
    if affine == 'unit':
        g, b = torch.ones(C), torch.zeros(C)
    res = torch.randn(G * M, C, generator=gen) * 2 if use_res else None
    mean, var, rstd, xhat, pre = _bn_ref64(x, g, b, 1e-5)
    ref = (pre.clamp_(min=0) if relu else pre).view(G * M, C)
    if use_res:
        ref = ref + res.double()
    y = torch.zeros(G * M, ld, dtype=ydt, device=tgt.device)
    # y2 is allocated with y's pitch and NaN-filled: the copy must land in the first G*M*C elements, at pitch C
    y2 = torch.full((G * M * ld,), float('nan'), dtype=_BF16, device=tgt.device) if use_y2 else None
    mean_k, rstd_k = ops.bn_train_fwd2(tgt.to(x.view(G * M, C)), tgt.to(g), tgt.to(b), y, M, C, 1e-5, relu, groups=G, res32=tgt.to(res),
                                       y2=y2, ldy=ld, coff=coff)
    # y: the fp32 result (3e-5, DT) or ONE bf16 rounding of it (4e-3: at most 2^-8 of the largest element)
    assert_close(y[:, coff:coff + C], ref, 3e-5 if ydt == _F32 else 4e-3, name='bn fwd2 y')
    assert not y[:, :coff].any().item() and not y[:, coff + C:].any().item(), 'columns outside the slice were written'
    assert_close(mean_k, mean, 1e-5, name='bn fwd2 mean')
    assert_close(rstd_k, rstd, 1e-5, name='bn fwd2 rstd')
    if use_y2:
        assert_close(y2[:G * M * C].view(G * M, C), ref, 4e-3, name='bn fwd2 y2')
        assert bool(y2[G * M * C:].isnan().all()), 'y2 written past its [rows, C] extent'


@pytest.mark.parametrize('ydt', [_F32, _BF16], ids=['y32', 'y16'])
def test_bn_train_fwd2_epilogue_statistics(tgt, ydt):
    """the stats_ws form: the statistics come from the producing GEMM's epilogue (ops.gemm(colstats=...)), no pass over x; checked
    against float64 statistics of the stored GEMM output, and the workspace comes back zeroed"""
    from cmda_amd import _lib as L
    torch.manual_seed(11)
    G, M, C, K, ld, coff = 3, 512, 72, 96, 96, 16
    a, w, bias = torch.randn(G * M, K), torch.randn(C, K), torch.randn(C) * 2 + 0.5
    ad, wd = tgt.to(a), tgt.to(w)
    ws = torch.zeros(G * int(L.lib().cmda_bn_ws_floats(C)), device=tgt.device)
    x = torch.empty(G * M, C, device=tgt.device)
    assert ops.colstats_ok(M, C)
    ops.gemm(ops.plain_view(ad, G * M, K), ops.plain_view(wd, C, K), x, G * M, C, K, dtype=0, bias=tgt.to(bias), colstats=(ws, M))
    assert ws.abs().max().item() > 0
    g, b = torch.rand(C) + 0.5, torch.randn(C)
    res = torch.randn(G * M, C)
    mean, var, rstd, xhat, pre = _bn_ref64(x.cpu().view(G, M, C), g, b, 1e-5)
    ref = pre.clamp_(min=0).view(G * M, C) + res.double()
    y = torch.zeros(G * M, ld, dtype=ydt, device=tgt.device)
    mean_k, rstd_k = ops.bn_train_fwd2(x, tgt.to(g), tgt.to(b), y, M, C, 1e-5, True, groups=G, res32=tgt.to(res), ldy=ld, coff=coff,
                                       stats_ws=ws)
    assert_close(y[:, coff:coff + C], ref, 3e-5 if ydt == _F32 else 4e-3, name='bn fwd2 (epilogue statistics) y')
    assert not y[:, :coff].any().item() and not y[:, coff + C:].any().item()
    assert_close(mean_k, mean, 1e-5, name='bn fwd2 (epilogue statistics) mean')
    assert_close(rstd_k, rstd, 1e-5, name='bn fwd2 (epilogue statistics) rstd')
    assert ws.abs().max().item() == 0.0, 'the workspace comes back zeroed'


@pytest.mark.parametrize('dt,tol', DT)
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('C', [40, 516])
@pytest.mark.parametrize('M', [1, 777, 40000])
def test_bn_apply(tgt, dt, tol, relu, M, C):
    """cmda_bn_apply (every eval-mode BatchNorm): y = relu?((x - mean) rstd gamma + beta) with given statistics, stored into a
    column slice, against float64"""
    gen = torch.Generator().manual_seed(M + C)
    ld, coff = C + 12, 8
    x = (torch.randn(M, C, generator=gen) * 2 + 3).to(dt)
    mean, rstd = torch.randn(C, generator=gen) + 3, torch.rand(C, generator=gen) + 0.3
    g, b = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.2
    ref = (x.double() - mean.double()) * rstd.double() * g.double() + b.double()
    ref = ref.clamp_(min=0) if relu else ref
    y = torch.zeros(M, ld, dtype=dt, device=tgt.device)
    ops.bn_apply(tgt.to(x), tgt.to(mean), tgt.to(rstd), tgt.to(g), tgt.to(b), y, M, C, relu, ld, coff)
    assert_close(y[:, coff:coff + C], ref, tol, name='bn apply')
    assert not y[:, :coff].any().item() and not y[:, coff + C:].any().item(), 'columns outside the slice were written'


# Conditioning of the one-pass variance.  The statistics pass accumulates sum d and sum d^2 of d = x - s around the shift s = row 0
# of the group (the contract in the header of batchnorm.hip) and forms var = E[d^2] - E[d]^2; the fused path (sums from a GEMM
# epilogue) has s = 0.  The cancellation loses a factor kappa = 1 + (mu - s)^2 / sigma^2, so the relative error of the variance is
# bounded by K * 2^-24 * kappa with kappa computed per channel from the float64 reference.  Dropping or breaking the shift fails the
# mu / sigma = 1000 case by six orders of magnitude.
# K: the worst err / (2^-24 kappa) over the sweep below against float64 was 5.121 on the emulator (ratio10_row0zero, sums) and 4.548 on
# an MI355X (the same case, two runs; fp32 atomics reorder the GPU's sums from run to run); K = 4 x the larger.  The two agree within 15 %:
# the constant is the rounding of sum d^2 and of E[d]^2, not of the summation order.  With row 0 an outlier (x ~ N(1000, 1) and row
# 0 = 0, or N(0, 1) and row 0 = 1000) the shift protects nothing: kappa = 4.1e3, the variance is 6.5e-4 off (rstd 3e-4) where torch's
# two-pass fp32 BatchNorm is at 1e-6 -- inside this bound, and stated here so that a rewrite changes it knowingly.
_BN_COND_K = 20.5
_BN_COND = {'ratio0': (0.0, None), 'ratio10': (10.0, None), 'ratio1000': (1000.0, None),
            'ratio0_row0zero': (0.0, 0.0), 'ratio10_row0zero': (10.0, 0.0), 'ratio1000_row0zero': (1000.0, 0.0),
            'ratio0_row0at1000': (0.0, 1000.0)}


@pytest.mark.parametrize('path', ['statistics_pass', 'epilogue_sums'])
@pytest.mark.parametrize('case', list(_BN_COND))
def test_batchnorm_conditioning(tgt, case, path):
    """fp32, no ReLU, 4096 x 64 against float64: x ~ N(mu, 1) with mu / sigma in {0, 10, 1000}, the same with row 0 replaced by 0, and
    N(0, 1) with row 0 = 1000; through the statistics pass (shift = row 0) and from epilogue sums (no shift).  The variance is read
    back from the saved rstd."""
    from cmda_amd import _lib as L
    M, C, eps = 4096, 64, 1e-5
    ratio, row0 = _BN_COND[case]
    gen = torch.Generator().manual_seed(int(ratio) + 1)
    x = torch.randn(M, C, generator=gen) + ratio      # N(mu, 1), mu / sigma = ratio
    if row0 is not None:
        x[0] = row0
    x64 = x.double()
    mu = x64.mean(0)
    var = ((x64 - mu) ** 2).mean(0)
    s = x64[0] if path == 'statistics_pass' else torch.zeros(C, dtype=torch.float64)
    kappa = 1 + (mu - s) ** 2 / var
    xd = tgt.to(x)
    y = torch.empty(M, C, device=tgt.device)
    ws = None
    if path == 'epilogue_sums':   # the workspace as a GEMM epilogue leaves it: [slot][sum | sum of squares][C], float64 sums rounded once
        ws = torch.zeros(int(L.lib().cmda_bn_ws_floats(C)))
        wv = ws.view(33, 2, C)
        for k, rows in enumerate(x64.chunk(32)):
            wv[k, 0], wv[k, 1] = rows.sum(0).float(), (rows * rows).sum(0).float()
        ws = tgt.to(ws)
    rm, rv = torch.zeros(C, device=tgt.device), torch.ones(C, device=tgt.device)
    mean_k, rstd_k = ops.bn_train_fwd(xd, tgt.to(torch.ones(C)), tgt.to(torch.zeros(C)), y, rm, rv, M, C, eps, 0.1, False, stats_ws=ws)
    var_k = rstd_k[0].double().cpu() ** -2 - eps
    worst = ((var_k - var).abs() / var / (2.0 ** -24 * kappa)).max().item()
    print(f'bn conditioning {case} {path} [{tgt.kind}]: worst var err / (2^-24 kappa) = {worst:.3f}, kappa max {kappa.max().item():.3g}, '
          f'rel var err max {((var_k - var).abs() / var).max().item():.3g}')
    if ws is not None:
        assert ws.abs().max().item() == 0.0, 'the workspace comes back zeroed'
    check_le('bn variance: relative error / (2^-24 kappa)', worst, _BN_COND_K)


# ------------------------------------------------------------------ entry points that had no test of their own, each against torch
@pytest.mark.parametrize('dt', [_F32, _BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('rows', [1, 33, 70001])
def test_copy2d(tgt, dt, rows):
    """cmda_copy2d: a [rows, cols] block between two row-major buffers of different pitch, both with a column offset; every element
    outside the block keeps its value (exact: the kernel only moves values)"""
    torch.manual_seed(rows)
    cols, src_ld, dst_ld, src_off, dst_off = 20, 28, 36, 4, 8
    src, dst0 = torch.randn(rows, src_ld).to(dt), torch.randn(rows, dst_ld).to(dt)
    dst = tgt.to(dst0.clone())
    ops.copy2d(tgt.to(src), dst, rows, cols, src_ld, dst_ld, src_off=src_off, dst_off=dst_off)
    want = dst0.clone()
    want[:, dst_off:dst_off + cols] = src[:, src_off:src_off + cols]
    assert torch.equal(dst.cpu(), want)


@pytest.mark.parametrize('dt', [_F32, _BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('n', [4, 1028, 4 << 20])
def test_cast_clear(tgt, dt, n):
    """cmda_cast_clear: the result is the cast of the fp32 source (one rounding for bf16: exact against torch's), the source is all
    zero afterwards"""
    torch.manual_seed(n)
    src = torch.randn(n)
    sd = tgt.to(src.clone())
    out = ops.cast_clear(sd, dt)
    assert out.dtype == dt and torch.equal(out.cpu(), src.to(dt))
    assert not sd.any().item(), 'the source is left zeroed'


@pytest.mark.parametrize('dt', [_F32, _BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('per_channel', [False, True], ids=['per_sample', 'per_sample_channel'])
@pytest.mark.parametrize('C', [8, 320])
def test_sample_scale(tgt, dt, per_channel, C):
    """cmda_sample_scale: x [B, H, W, C] times scale[b] or scale[b, c] (one fp32 product, rounded once for bf16: exact)"""
    torch.manual_seed(C)
    B, H, W = 3, 7, 5
    x = torch.randn(B, H, W, C).to(dt)
    sc = torch.rand(B, C) + 0.5 if per_channel else torch.rand(B) + 0.5
    want = (x.float() * (sc.view(B, 1, 1, C) if per_channel else sc.view(B, 1, 1, 1))).to(dt)
    out = ops.sample_scale(tgt.to(x), tgt.to(sc), B, C, per_channel=per_channel)
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize('nc', [19, 7])
@pytest.mark.parametrize('h,w,H,W', [(8, 8, 32, 32), (6, 10, 24, 40), (7, 5, 28, 20), (8, 8, 8, 8), (5, 7, 13, 18), (2, 3, 32, 48), (9, 17, 36, 68),
                                     (12, 20, 24, 40), (10, 9, 30, 27), (32, 40, 128, 160), (11, 13, 66, 65)])
def test_upsample_logits_nchw(tgt, h, w, H, W, nc):
    """cmda_upsample_logits_nchw (the checker of test_dacs.py / test_image_uda.py, checked itself here) against F.interpolate at the
    size pairs of test_ce_upsample: integer and non-integer ratios, identity"""
    torch.manual_seed(h * 3 + w + nc)
    logits = torch.randn(2, h, w, nc) * 2
    ref = F.interpolate(logits.double().permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=False)
    out = ops.upsample_logits_nchw(tgt.to(logits), H, W)
    assert out.shape == (2, nc, H, W)
    # torch's own fp32 F.interpolate is up to 1.04e-6 of the largest element off the float64 reference at these sizes (the non-integer
    # ratios: the fp32 source coordinate), the kernel 1.06e-6 on an MI355X; the bound is 4 x torch's
    assert_close(out, ref, 4e-6, name='upsample logits nchw')


def _permute_desc(n):
    import numpy as np
    return np.zeros(n, dtype=[('src', '<u8'), ('dst', '<u8'), ('d', '<i4', 4), ('p', '<i4', 4), ('flip', '<i4'), ('mode', '<i4'),
                              ('total', '<i8')])


def test_permute4_batch(tgt):
    """cmda_permute4_batch, all three code paths in ONE launch over tensors of different shapes.  General path: axis flips; channel
    padding (Ci = 3 -> 8, bf16 and fp32 destination, padded entries zero); a (0, 2, 3, 1) permutation whose total is not a multiple
    of 4.  Fast path: (0, 2, 3, 1) with an aligned source and a total that is.  Drain mode (records built by ops._conv_drain_plan):
    gradient += shadow in [Co, Ci, KH, KW] order, shadow cleared; with and without channel-padded shadows, totals that are not
    multiples of 4 or of the 1024-element chunk, and an all-zero shadow that leaves its gradient bit-identical."""
    import numpy as np
    torch.manual_seed(12)
    dev = tgt.device
    keep, recs, checks = [], [], []

    def plain(src, dims, perm, flip, dst_dt, want):
        """one non-drain record; dims = the (padded) dims the destination is laid out with"""
        s = tgt.to(src.contiguous())
        dst = torch.full(want.shape, float('nan'), dtype=dst_dt, device=dev)
        keep.extend([s, dst])
        recs.append((s.data_ptr(), dst.data_ptr(), tuple(dims), tuple(perm), flip, int(dst_dt == _BF16), want.numel()))
        checks.append((dst, want.to(dst_dt)))

    w = torch.randn(6, 5, 3, 3)
    plain(w, (6, 5, 3, 3), (1, 2, 3, 0), 0b1100, _F32, w.flip(2, 3).permute(1, 2, 3, 0).contiguous())     # general, flips
    plain(w, (6, 5, 3, 3), (1, 2, 3, 0), 0b1100, _BF16, w.flip(2, 3).permute(1, 2, 3, 0).contiguous())
    w3 = torch.randn(16, 3, 7, 7)                                                                           # general, Ci 3 -> 8
    padded = torch.zeros(16, 7, 7, 8)
    padded[..., :3] = w3.permute(0, 2, 3, 1)
    plain(w3, (16, 8, 7, 7), (0, 2, 3, 1), (2 << 8) | (3 << 16), _BF16, padded)
    plain(w3, (16, 8, 7, 7), (0, 2, 3, 1), (2 << 8) | (3 << 16), _F32, padded)
    wf = torch.randn(8, 33, 3, 3)                                                                           # fast path: 2376 = 4 * 594
    assert wf.numel() % 4 == 0 and wf.numel() % 1024
    plain(wf, (8, 33, 3, 3), (0, 2, 3, 1), 0, _F32, wf.permute(0, 2, 3, 1).contiguous())
    plain(wf, (8, 33, 3, 3), (0, 2, 3, 1), 0, _BF16, wf.permute(0, 2, 3, 1).contiguous())
    wg = torch.randn(7, 5, 3, 3)                                                                            # same permutation, total 315: general
    assert wg.numel() % 4
    plain(wg, (7, 5, 3, 3), (0, 2, 3, 1), 0, _F32, wg.permute(0, 2, 3, 1).contiguous())
    assert all(k.data_ptr() % 16 == 0 for k in keep)
    # drain records: (gradient shape, padded channel count of the shadow or 0, all-zero shadow)
    drains = []
    for (Co, Ci, KH, KW), cs, zero in [((16, 3, 7, 7), 8, False), ((5, 7, 3, 3), 0, False), ((64, 40, 3, 3), 0, False),
                                       ((9, 3, 3, 3), 4, False), ((6, 5, 3, 3), 0, True)]:
        cs = cs or Ci
        sh = torch.zeros(Co, KH, KW, cs) if zero else torch.randn(Co, KH, KW, cs)   # (the padded channels carry GEMM sums too)
        g0 = torch.randn(Co, Ci, KH, KW)
        if zero:
            g0[0, 0, 0, 0] = -0.0   # (a stored sum would turn it into +0)
        shd, gd = tgt.to(sh.view(Co, KH * KW * cs).clone()), tgt.to(g0.clone())
        drains.append((sh, g0, shd, gd, Ci, cs, zero))
    assert [d[1].numel() % 4 != 0 for d in drains].count(True) >= 2 and all(d[1].numel() % 1024 for d in drains)
    dtab, dblk, dn = ops._conv_drain_plan(dev, [(d[2], d[3]) for d in drains])
    drec = dtab.cpu().numpy().view(_permute_desc(1).dtype)
    desc = _permute_desc(len(recs) + len(drec))
    for i, r in enumerate(recs):
        desc[i] = r
    desc[len(recs):] = drec
    blocks = [(i, c) for i, r in enumerate(recs) for c in range((r[6] + 1023) // 1024)]
    dblocks = dblk.cpu().numpy().view(np.int32).reshape(-1, 2).copy()
    assert len(dblocks) == dn
    dblocks[:, 0] += len(recs)
    blocks = np.concatenate([np.asarray(blocks, dtype=np.int32), dblocks])
    tab = tgt.to(torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()))
    blk = tgt.to(torch.from_numpy(blocks.copy()))
    ops.permute4_batch(tab, blk, len(blocks))
    for dst, want in checks:
        assert torch.equal(dst.cpu(), want)          # moves (and rounds once for bf16): exact
    for sh, g0, shd, gd, Ci, cs, zero in drains:
        Co, _, KH, KW = g0.shape
        want = g0 + sh[..., :Ci].permute(0, 3, 1, 2)  # one fp32 addition per element: exact
        if zero:
            assert torch.equal(gd.cpu().view(torch.int32), g0.view(torch.int32)), 'an all-zero shadow must leave the gradient bit-identical'
        else:
            assert torch.equal(gd.cpu(), want)
        assert not shd.view(Co, KH, KW, cs)[..., :Ci].any().item(), 'the shadow is left zeroed in its real channels'


def test_layernorm_deferred_parameter_gradients(tgt):
    """the deferred form of cmda_layernorm_bwd2 (dgamma == NULL: the partial sums stay in the layer's workspace) and
    cmda_layernorm_fold_batch: inside ops.backward_scope several layers of different width (C = 1024 needs four 256-channel
    chunks, whose blocks return early for the narrow layers), one of them with two backward calls before the fold, dgamma / dbeta
    pre-filled; after the scope they hold the float64 sums and every layer's workspace is zero.  The immediate form gives the same."""
    from cmda_amd import deferred as D
    torch.manual_seed(21)
    layers = []
    for C, rows, calls in [(32, 37, 1), (320, 9001, 2), (1024, 37, 1), (32, 9001, 1), (1024, 9001, 1)]:
        g = torch.randn(C)
        xs = [torch.randn(rows, C) * 2 + 1 for _ in range(calls)]
        dys = [torch.randn(rows, C) for _ in range(calls)]
        dg0, db0 = torch.randn(C), torch.randn(C)
        dgr, dbr = dg0.double(), db0.double()
        for x, dy in zip(xs, dys):
            x64 = x.double()
            mu = x64.mean(1, keepdim=True)
            xhat = (x64 - mu) * (((x64 - mu) ** 2).mean(1, keepdim=True) + 1e-6).rsqrt()
            dgr, dbr = dgr + (dy.double() * xhat).sum(0), dbr + dy.double().sum(0)
        layers.append(dict(C=C, g=tgt.to(g), xs=[tgt.to(x) for x in xs], dys=[tgt.to(d) for d in dys], dg0=dg0, db0=db0, dgr=dgr, dbr=dbr))

    def run(deferred):
        out = []
        for l in layers:
            l['dg'], l['db'] = tgt.to(l['dg0'].clone()), tgt.to(l['db0'].clone())
            out.append((l['dg'], l['db']))
        for l in layers:
            for x, dy in zip(l['xs'], l['dys']):
                _, mean, rstd = ops.layernorm_fwd(x, l['g'], torch.zeros_like(l['g']), 1e-6)
                ops.layernorm_bwd(dy, x, l['g'], mean, rstd, l['dg'], l['db'])
                if deferred:
                    assert torch.equal(l['dg'].cpu(), l['dg0']), 'deferred: nothing reaches dgamma before the fold'
        return out

    D.reset()
    with ops.backward_scope():
        got = run(True)
        regions = [D.LN.regions[dg.data_ptr()] for dg, _ in got]
        assert all(r[0].abs().max().item() > 0 for r in regions)
    for l, (dg, db), r in zip(layers, got, regions):
        assert_close(dg, l['dgr'], 2e-5, name=f'deferred ln dgamma C={l["C"]}')    # (the bounds of test_layernorm)
        assert_close(db, l['dbr'], 2e-5, name=f'deferred ln dbeta C={l["C"]}')
        assert r[0].abs().max().item() == 0.0, 'the fold leaves every region zeroed'
    deferred = [(dg.cpu(), db.cpu()) for dg, db in got]
    for l, (dg, db), (dg_d, db_d) in zip(layers, run(False), deferred):
        assert_close(dg, l['dgr'], 2e-5, name=f'immediate ln dgamma C={l["C"]}')
        assert_close(dg, dg_d, 2e-5, name=f'ln dgamma: immediate against deferred C={l["C"]}')
        assert_close(db, db_d, 2e-5, name=f'ln dbeta: immediate against deferred C={l["C"]}')


@pytest.mark.parametrize('dt,tol', DT)
def test_layernorm_single_dtype_entry_points(tgt, dt, tol):
    """cmda_layernorm_fwd / cmda_layernorm_bwd: the one-dtype forms of the ABI (no Python wrapper calls them) against float64, and
    the queries the backward's workspace is sized with: cmda_layernorm_slots x 2 x C = cmda_layernorm_bwd_ws_floats"""
    from cmda_amd import _lib as L
    torch.manual_seed(8)
    rows, C = 301, 160
    x, dy = (torch.randn(rows, C) * 2 + 1).to(dt), torch.randn(rows, C).to(dt)
    g, b = torch.randn(C), torch.randn(C)
    x64 = x.double()
    mu = x64.mean(1, keepdim=True)
    rs = (((x64 - mu) ** 2).mean(1, keepdim=True) + 1e-6).rsqrt()
    xhat = (x64 - mu) * rs
    gy = dy.double() * g.double()
    dxref = rs * (gy - gy.mean(1, keepdim=True) - xhat * (gy * xhat).mean(1, keepdim=True))
    xd, dyd, gd, bd = map(tgt.to, (x, dy, g, b))
    y = torch.empty_like(xd)
    mean, rstd = torch.empty(rows, device=tgt.device), torch.empty(rows, device=tgt.device)
    st = L.stream_of(xd)
    L.call('cmda_layernorm_fwd', L.ptr(xd), L.ptr(gd), L.ptr(bd), L.ptr(y), L.ptr(mean), L.ptr(rstd), L.c_i64(rows), L.c_i32(C),
           L.c_f32(1e-6), L.dtype_tag(xd), st)
    assert_close(y, xhat * g.double() + b.double(), tol, name='ln fwd (one-dtype entry point)')
    assert_close(mean, mu[:, 0], 1e-5, name='ln mean (one-dtype entry point)')
    slots = int(L.lib().cmda_layernorm_slots())
    assert slots > 0 and slots * 2 * C == int(L.lib().cmda_layernorm_bwd_ws_floats(rows, C))
    ws = torch.zeros(slots * 2 * C, device=tgt.device)
    dx = torch.empty_like(dyd)
    dg, db = torch.zeros(C, device=tgt.device), torch.zeros(C, device=tgt.device)
    L.call('cmda_layernorm_bwd', L.ptr(dyd), L.ptr(xd), L.ptr(gd), L.ptr(mean), L.ptr(rstd), None, L.ptr(dx), L.ptr(dg), L.ptr(db),
           L.ptr(ws), L.c_i64(rows), L.c_i32(C), None, L.c_i64(0), None, L.dtype_tag(xd), st)
    assert_close(dx, dxref, tol, name='ln dx (one-dtype entry point)')
    assert_close(dg, (dy.double() * xhat).sum(0), 2e-5, name='ln dgamma (one-dtype entry point)')
    assert_close(db, dy.double().sum(0), 2e-5, name='ln dbeta (one-dtype entry point)')
    assert ws.abs().max().item() == 0.0, 'the workspace is zero again when the call completes'
