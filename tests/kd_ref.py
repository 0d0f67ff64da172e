"""The distillation loss of svnet_amd/csrc/kdloss.hip restated in float64 torch on the CPU (the yardstick of tests/test_hip_kd.py):

    ce_r = -sum_c soft_rc log_softmax(s_r)_c,  soft_rc = 1 - eps at c == y_r, eps / (C - 1) elsewhere        (utils.py:33-50)
    kl_r = sum_c p_rc (logp_rc - logq_rc),  logp = log_softmax(t_r / T), logq = log_softmax(s_r / T), p = exp(logp)
    L = (1 - alpha) mean_r ce_r + alpha T^2 mean_r kl_r,  dL/ds by autograd

The reference repository publishes distilled checkpoints but no distillation source, so the definition is Hinton et al.'s; it is
cross-checked against torch's own kl_div and, at alpha = 0, against the oracle's cal_loss (tests/test_host_kd.py).
"""
import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


def _rows(x):
    """[R,C] as it is; [B,C,N] -> [B*N,C] (rows = points)."""
    return x if x.dim() == 2 else x.permute(0, 2, 1).reshape(-1, x.shape[1])


def kd_terms(s, t, y, T, alpha, eps):
    """(L, CE, KL) as float64 tensors; s may require grad.  s, t: [R,C] or [B,C,N]; y: [R] or [B,N]."""
    s2, t2 = _rows(s.to(F64)), _rows(t.to(F64))
    R, C = s2.shape
    soft = torch.full((R, C), eps / (C - 1), dtype=F64)
    soft.scatter_(1, y.reshape(-1, 1), 1 - eps)
    ce = -(soft * torch.log_softmax(s2, dim=1)).sum(1).mean()
    logp, logq = torch.log_softmax(t2 / T, dim=1), torch.log_softmax(s2 / T, dim=1)
    kl = (logp.exp() * (logp - logq)).sum(1).mean()
    return (1 - alpha) * ce + alpha * T * T * kl, ce, kl


def kd_reference(s, t, y, T, alpha, eps, upstream=1.0):
    """{"out0": [L, CE, KL], "dx0": upstream * dL/ds in the layout of s} as float64 numpy arrays."""
    s6 = s.detach().to(F64).clone().requires_grad_(True)
    L, ce, kl = kd_terms(s6, t.detach(), y, T, alpha, eps)
    L.backward(torch.tensor(float(upstream), dtype=F64))
    return {"out0": np.array([float(L.detach()), float(ce.detach()), float(kl.detach())]), "dx0": s6.grad.numpy()}


def kd_gradient_formula(s, t, y, T, alpha, eps):
    """The closed form of dL/ds the kernel evaluates, float64, rows layout."""
    s, t = s.to(F64), t.to(F64)
    R, C = s.shape
    soft = torch.full((R, C), eps / (C - 1), dtype=F64)
    soft.scatter_(1, y.reshape(-1, 1), 1 - eps)
    return ((1 - alpha) * (torch.softmax(s, 1) - soft) + alpha * T * (torch.softmax(s / T, 1) - torch.softmax(t / T, 1))) / R


def torch_kl_term(s, t, T):
    """T^2 KL through torch's own kl_div (the usual way the term is written in training scripts)."""
    s, t = s.to(F64), t.to(F64)
    return F.kl_div(torch.log_softmax(s / T, dim=1), torch.softmax(t / T, dim=1), reduction="batchmean") * T * T


def make_logits(gen, R, C, phase=0):
    """[R,C] logits like run_smooth_ce's (tests/test_hip_kernel_tiers.py): scale 30, clamped to +-80, with planted +-80 columns (the
    rows chosen by `phase`: student and teacher plant theirs independently) - softmax probabilities underflow to exactly 0 in fp32."""
    x = torch.clamp(torch.randn(R, C, generator=gen) * 30, -80, 80)
    x[phase % 3::3, 0] = 80.0
    x[(phase + 1) % 3::3, C - 1] = -80.0
    return x


def make_targets(gen, R, C):
    y = torch.randint(0, C, (R,), generator=gen)
    y[::4] = 0
    y[1::4] = C - 1
    return y


def channel_major(rows, B, N):
    """[B*N,C] rows -> the contiguous [B,C,N] tensor holding the same values (row b*N + n = point n of cloud b)."""
    return rows.view(B, N, rows.shape[1]).permute(0, 2, 1).contiguous()
