"""The dil = 1 row walk of dwconv.hip (MixFFN depthwise convolution: forward + GELU, data gradient, fused GELU backward) against plain
torch fp32 at test_kernels.test_dwconv's tolerances, and bit for bit against the row-run kernels it replaces (CMDA_DW_BAND=0 selects
those; CMDA_DW_BAND=n fixes the walk's band height, so that band boundaries fall where a test wants them)."""
import pytest
import torch
import torch.nn.functional as F

from cmda_amd import ops
from conftest import assert_close

DT = [(torch.float32, 3e-5), (torch.bfloat16, 1.6e-2)]

# (B, H, W, C).  The walk serves bf16: 4 columns per thread (2 in the fused backward), 4 channels per lane, 64 (fused: 16) lanes of
# channels per workgroup, a band passed over four rows at a time.  fp32 (parity mode) stays on the row-run kernels, which every case
# checks against torch all the same.
SHAPES = [
    (2, 13, 8, 24),    # H not a multiple of any band; C = 4 * 6 < a channel group
    (1, 5, 40, 260),   # H smaller than the default band; C = 4 * 65: odd quad count, one lane past a 64-quad group
    (1, 1, 8, 12),     # H = 1: every row of the window but one is padding
    (2, 19, 4, 36),    # W = one bf16 run: both halo columns are padding
    (1, 37, 12, 68),   # several bands + a ragged one; W = 3 runs; C = 4 * 17 crosses a 16-quad group
    (3, 8, 16, 8),     # H = exactly one band of 8; 3 images
    (1, 6, 2, 8),      # W below a run: the row-run kernels take forward and dx, the walk the fused backward
    (2, 7, 9, 16),     # odd width: row-run kernels
]
BANDS = [None, 1, 3, 4, 5, 16]


def _case(seed, shape, dt):
    torch.manual_seed(seed)
    B, H, W, C = shape
    x = torch.randn(B, H, W, C).to(dt)
    w, b = torch.randn(C, 1, 3, 3) * 0.3, torch.randn(C)
    dy = torch.randn(B, H, W, C).to(dt)
    prev = torch.randn(B, H, W, C).to(dt)
    return x, w, b, dy, prev


def _torch_ref(x, w, b, dy, act):
    C = x.shape[-1]
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    z = F.conv2d(xr, wr, br if act else None, padding=1, groups=C)
    y = F.gelu(z) if act == 'gelu' else z
    y.backward(dy.float().permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1), wr.grad.view(C, 9), br.grad if act else None


def _run(tgt, x, w, b, dy, prev, act):
    """every dil = 1 entry point once: y, dz (fused), dx of dz, dx accumulated onto prev, dw, dbias"""
    B, H, W, C = x.shape
    xd, wd, bd, dyd = tgt.to(x), tgt.to(w.view(C, 9).t().contiguous()), tgt.to(b) if act else None, tgt.to(dy)
    y = ops.dwconv_fwd(xd, wd, bd, B, H, W, C, 1, act)
    dw, db = torch.zeros(C, 9, device=tgt.device), torch.zeros(C, device=tgt.device)
    dz = ops.dwconv_gelu_bwd_fused(xd, wd, bd, dyd, dw, db, B, H, W, C, 1) if act == 'gelu' else dyd
    dx = ops.dwconv_bwd_data(dz, wd, B, H, W, C, 1)
    acc = ops.dwconv_bwd_data(dz, wd, B, H, W, C, 1, out=tgt.to(prev.clone()), accumulate=True)
    return y, dz, dx, acc, dw, db


@pytest.mark.parametrize('dt,tol', DT)
@pytest.mark.parametrize('band', BANDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_walk_against_torch(tgt, monkeypatch, dt, tol, band, shape):
    if band is None:
        monkeypatch.delenv('CMDA_DW_BAND', raising=False)
    else:
        monkeypatch.setenv('CMDA_DW_BAND', str(band))
    for act in ('gelu', None):
        x, w, b, dy, prev = _case(shape[1] * 100 + shape[2], shape, dt)
        ry, rdx, rdw, rdb = _torch_ref(x, w, b, dy, act)
        y, dz, dx, acc, dw, db = _run(tgt, x, w, b, dy, prev, act)
        assert_close(y, ry, tol, name='dw fwd')
        assert_close(dx, rdx, tol * 2, name='dw dx')
        assert_close(acc, rdx + prev.float(), tol * 3, name='dw dx accumulate')
        if act == 'gelu':
            B, H, W, C = shape
            prep = ops.dwconv_gelu_bwd_prep(tgt.to(x), tgt.to(w.view(C, 9).t().contiguous()), tgt.to(b), tgt.to(dy), B, H, W, C, 1)
            assert_close(dz, prep, 1e-6 if dt == torch.float32 else 4e-3, name='fused dz against the backward prep')
            assert_close(dw, rdw, tol, name='fused dweight')
            assert_close(db, rdb, tol, name='fused dbias')


@pytest.mark.parametrize('dt,tol', DT)
@pytest.mark.parametrize('band', [None, 3, 16])
@pytest.mark.parametrize('shape', SHAPES)
def test_walk_equals_row_run(tgt, monkeypatch, dt, tol, band, shape):
    """y, dz and dx of the walk are the row-run kernels' bit for bit (same tap order, same epilogues); dw / dbias are sums of the same
    terms in another order and are checked against torch above"""
    x, w, b, dy, prev = _case(7 + shape[1], shape, dt)
    monkeypatch.setenv('CMDA_DW_BAND', '0')
    old = _run(tgt, x, w, b, dy, prev, 'gelu')
    old_lin = _run(tgt, x, w, b, dy, prev, None)
    if band is None:
        monkeypatch.delenv('CMDA_DW_BAND')
    else:
        monkeypatch.setenv('CMDA_DW_BAND', str(band))
    new = _run(tgt, x, w, b, dy, prev, 'gelu')
    new_lin = _run(tgt, x, w, b, dy, prev, None)
    for name, a, o in zip(('y', 'dz', 'dx', 'dx accumulate'), new[:4], old[:4]):
        assert torch.equal(a, o), f'{name}: walk differs from the row-run kernel'
    for name, a, o in zip(('y', 'dz', 'dx', 'dx accumulate'), new_lin[:4], old_lin[:4]):
        assert torch.equal(a, o), f'{name} (no activation): walk differs from the row-run kernel'


@pytest.mark.parametrize('dt,tol', DT)
def test_walk_accumulates_into_dw(tgt, monkeypatch, dt, tol):
    """dw / dbias are ADDED to (the optimizer's flat gradient store is not zeroed per layer)"""
    monkeypatch.delenv('CMDA_DW_BAND', raising=False)
    shape = (2, 9, 8, 40)
    B, H, W, C = shape
    x, w, b, dy, _ = _case(3, shape, dt)
    _, _, rdw, rdb = _torch_ref(x, w, b, dy, 'gelu')
    dw0, db0 = torch.randn(C, 9), torch.randn(C)
    dw, db = tgt.to(dw0.clone()), tgt.to(db0.clone())
    ops.dwconv_gelu_bwd_fused(tgt.to(x), tgt.to(w.view(C, 9).t().contiguous()), tgt.to(b), tgt.to(dy), dw, db, B, H, W, C, 1)
    assert_close(dw, dw0 + rdw, tol, name='fused dweight accumulated')
    assert_close(db, db0 + rdb, tol, name='fused dbias accumulated')
