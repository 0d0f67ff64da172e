"""CPU tests of the distillation loss's host side: the float64 restatement tests/kd_ref.py against torch's kl_div, the oracle's cal_loss
and a finite difference; the pure-host shape queries of svnet_amd/csrc/loss.hip; argument validation that needs no device."""
import numpy as np
import pytest
import torch

from oracle import sv_ref
from tests import kd_ref as K

F64 = torch.float64


def _case(R=9, C=7, seed=5):
    g = torch.Generator().manual_seed(seed)
    return K.make_logits(g, R, C, 0), K.make_logits(g, R, C, 1), K.make_targets(g, R, C)


@pytest.mark.parametrize("T", [0.5, 1.0, 4.0])
def test_reference_kl_term_is_torch_kl_div(T):
    s, t, y = _case()
    _, _, kl = K.kd_terms(s, t, y, T, 0.5, 0.2)
    want = float(K.torch_kl_term(s, t, T))
    assert np.isfinite(want) and abs(float(kl) * T * T - want) <= 1e-12 * max(1.0, abs(want))


@pytest.mark.parametrize("smoothing", [True, False])
def test_reference_at_alpha_zero_is_the_oracles_cal_loss(smoothing):
    s, t, y = _case(R=12, C=40)
    eps = 0.2 if smoothing else 0.0
    L, ce, _ = K.kd_terms(s, t, y, 4.0, 0.0, eps)
    want = float(sv_ref.cal_loss(s.double(), y, smoothing=smoothing))
    assert float(L) == float(ce) and abs(float(L) - want) <= 1e-12 * max(1.0, abs(want))
    # and in the channel-major layout: rows = points
    B, N = 3, 4
    L3, _, _ = K.kd_terms(K.channel_major(s, B, N), K.channel_major(t, B, N), y.view(B, N), 4.0, 0.0, eps)
    assert abs(float(L3) - want) <= 1e-12 * max(1.0, abs(want))


def test_reference_gradient_against_a_central_difference_and_the_closed_form():
    g = torch.Generator().manual_seed(11)
    s, t = torch.randn(3, 5, generator=g, dtype=F64) * 2, torch.randn(3, 5, generator=g, dtype=F64) * 2
    y = torch.tensor([0, 4, 2])
    T, alpha, eps = 4.0, 0.5, 0.2
    ref = K.kd_reference(s, t, y, T, alpha, eps)
    h = 1e-6
    fd = np.zeros((3, 5))
    for r in range(3):
        for c in range(5):
            d = torch.zeros(3, 5, dtype=F64)
            d[r, c] = h
            fd[r, c] = (float(K.kd_terms(s + d, t, y, T, alpha, eps)[0]) - float(K.kd_terms(s - d, t, y, T, alpha, eps)[0])) / (2 * h)
    assert np.abs(fd - ref["dx0"]).max() <= 1e-8 * np.abs(ref["dx0"]).max()
    assert np.abs(K.kd_gradient_formula(s, t, y, T, alpha, eps).numpy() - ref["dx0"]).max() <= 1e-14
    # the layouts agree: the channel-major gradient is the rows gradient, transposed back
    B, N = 1, 3
    ref3 = K.kd_reference(K.channel_major(s, B, N), K.channel_major(t, B, N), y.view(B, N), T, alpha, eps, upstream=1.7)
    assert np.abs(ref3["dx0"] - 1.7 * K.channel_major(torch.from_numpy(ref["dx0"]), B, N).numpy()).max() <= 1e-14
    assert np.abs(ref3["out0"] - ref["out0"]).max() <= 1e-14


def test_underflowing_teacher_probabilities_are_finite_in_the_reference():
    s, t, y = _case(R=30, C=2)
    ref = K.kd_reference(s, t, y, 0.5, 1.0, 0.0)
    assert np.isfinite(ref["out0"]).all() and np.isfinite(ref["dx0"]).all()
    assert float(torch.softmax(t.float() / 0.5, 1).min()) == 0.0          # (the case does underflow in fp32)


def test_supported_and_tier_queries_answer_without_a_gpu():
    from svnet_amd import _lib
    L = _lib.lib()
    ROWS, CM = _lib.KD_ROWS, _lib.KD_CHANNEL_MAJOR
    for args in ((ROWS, 1, 2, 1), (ROWS, 32, 40, 1), (ROWS, 65536, 50, 1), (CM, 32, 50, 2048), (CM, 1, 2, 1), (CM, 2, 130, 1025)):
        assert L.svnet_kd_supported(*args) == 1 and L.svnet_kd_tier(*args) >= 0, args
    for args in ((ROWS, 0, 40, 1), (ROWS, 4, 1, 1), (ROWS, 4, 40, 2), (ROWS, 4, 65537, 1), (ROWS, 1 << 31, 40, 1), (CM, 0, 50, 8),
                 (CM, 2, 50, 0), (CM, 2, 1, 8), (CM, 1 << 16, 50, 1 << 15), (CM, 2, -3, 8), (2, 4, 40, 1), (-1, 4, 40, 1)):
        assert L.svnet_kd_supported(*args) == 0 and L.svnet_kd_tier(*args) == -1, args
    # tiers are monotone in the classes and in the rows, and every supported shape has one
    for layout, n in ((ROWS, 1), (CM, 16)):
        for rows in (1, 4096, 1 << 20):
            tiers = [L.svnet_kd_tier(layout, rows, C, n) for C in range(2, 400)]
            assert min(tiers) >= 0 and all(b >= a for a, b in zip(tiers, tiers[1:])), (layout, rows)
        for C in (2, 50, 130):
            tiers = [L.svnet_kd_tier(layout, 1 << e, C, n) for e in range(0, 26)]
            assert min(tiers) >= 0 and all(b >= a for a, b in zip(tiers, tiers[1:])), (layout, C)
    # channel-major tiers depend on the number of points B * N, not on how it splits
    assert L.svnet_kd_tier(CM, 1 << 10, 50, 1 << 10) == L.svnet_kd_tier(CM, 1, 50, 1 << 20) == L.svnet_kd_tier(CM, 1 << 20, 50, 1)
    # the call itself refuses what the query refuses, with a message, before it touches any pointer's memory
    one = 1
    assert L.svnet_kd_loss_f32(CM, one, one, one, 2, 1, 5, 0.2, 0.5, 4.0, one, None, one, 8192, None) == -2
    assert b"not taken" in L.svnet_last_error()
    assert L.svnet_kd_loss_f32(ROWS, one, one, one, 2, 40, 1, 0.2, 0.5, 0.0, one, None, one, 8192, None) == -1
    assert L.svnet_kd_loss_f32(ROWS, one, one, one, 2, 40, 1, 0.2, 1.5, 4.0, one, None, one, 8192, None) == -1
    assert L.svnet_kd_loss_f32(ROWS, one, one, one, 2, 40, 1, 0.2, 0.5, 4.0, one, None, one, 100, None) == -3
    assert L.svnet_kd_loss_f32(ROWS, None, one, one, 2, 40, 1, 0.2, 0.5, 4.0, one, None, one, 8192, None) == -1


def test_argument_errors_need_no_device():
    from svnet_amd.train import Distiller, kd_loss, kd_seg_loss
    s, t, y = torch.zeros(4, 40), torch.zeros(4, 40), torch.zeros(4, dtype=torch.int64)
    s3, t3, y3 = torch.zeros(2, 50, 8), torch.zeros(2, 50, 8), torch.zeros(2, 8, dtype=torch.int64)
    for fn, a in ((kd_loss, (s, t, y)), (kd_seg_loss, (s3, t3, y3))):
        for T in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="temperature"):
                fn(*a, T=T)
        for alpha in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match="alpha"):
                fn(*a, alpha=alpha)
        with pytest.raises(TypeError, match="numbers"):
            fn(*a, T="hot")
        with pytest.raises(ValueError, match="cuda"):                      # CPU tensors: no fallback
            fn(*a)
        with pytest.raises(TypeError, match="tensors"):
            fn(a[0], a[1].numpy(), a[2])
        with pytest.raises(TypeError, match="float32"):
            fn(a[0], a[1].double(), a[2])
        with pytest.raises(TypeError, match="int64"):
            fn(a[0], a[1], a[2].int())
        with pytest.raises(ValueError, match="differ in shape"):
            fn(a[0], a[1][:, :-1], a[2])
        with pytest.raises(ValueError, match="one class per row"):
            fn(a[0], a[1], a[2][:1])
    with pytest.raises(ValueError, match=r"\[R,C\]"):
        kd_loss(s3, t3, y3)
    with pytest.raises(ValueError, match=r"\[B,C,N\]"):
        kd_seg_loss(s, t, y)
    lin = torch.nn.Linear(3, 2)
    with pytest.raises(ValueError, match="temperature"):
        Distiller(lin, (s,), T=0.0)
    with pytest.raises(ValueError, match="alpha"):
        Distiller(lin, (s,), alpha=2.0)
    with pytest.raises(TypeError, match="Module"):
        Distiller(lambda x: x, (s,))
    with pytest.raises(TypeError, match="inputs"):
        Distiller(lin, ())
    d = Distiller(lin.train(), (s,), T=2.0, alpha=0.25)
    assert not lin.training and not any(p.requires_grad for p in lin.parameters()) and (d.T, d.alpha) == (2.0, 0.25)
    with pytest.raises(RuntimeError, match="run"):
        d.loss_fn(s, y)
