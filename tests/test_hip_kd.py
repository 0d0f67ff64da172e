"""GPU tests (-m gpu) of the distillation loss (svnet_amd/csrc/loss.hip through svnet_amd.train.kd_loss / kd_seg_loss) against the
float64 restatement tests/kd_ref.py, and of a teacher run beside a student's train step (svnet_amd.train.Distiller, train_epoch).

Bounds are the loss family's own (tests/test_hip_kernel_tiers.py): {L, CE, KL} at OUT_RTOL of max(|reference|, 1), dlogits at GRAD_RTOL of
the tensor's max.  Shapes on both sides of every dispatch edge are read from svnet_kd_tier, never copied."""
import functools

import numpy as np
import pytest
import torch

from tests import kd_ref as K
from tests.golden import cases as C
from tests.test_hip_train_parity import TRAIN_CASES, build_model

pytestmark = pytest.mark.gpu

OUT_RTOL = 1e-5
GRAD_RTOL = 1e-4
UPSTREAM = 1.7
# (T, alpha, eps)
PARAMS = [(1.0, 0.3, 0.2), (4.0, 0.5, 0.2), (0.5, 1.0, 0.0), (4.0, 0.0, 0.2)]
PARAM_IDS = ["T%g_a%g_e%g" % p for p in PARAMS]


def _lib():
    from svnet_amd import _lib as L
    return L


def _tier(layout, B, Cn, N):
    return _lib().lib().svnet_kd_tier(layout, B, Cn, N)


def _edges(f, lo, hi):
    """Every x in lo .. hi-1 with f(x) != f(x + 1), f monotone (asserted by tests/test_host_kd.py): bisection per step of f."""
    out = []
    while f(lo) != f(hi):
        a, b = lo, hi
        while b - a > 1:
            m = (a + b) // 2
            a, b = (m, b) if f(m) == f(lo) else (a, m)
        out.append(a)
        lo = b
    return out


def _rows_cases():
    rows = _lib().KD_ROWS
    cases = [(1, 2), (7, 65), (4097, 40), (4097, 130)]
    for e in _edges(lambda c: _tier(rows, 7, c, 1), 2, 4096):
        cases += [(7, e), (7, e + 1)]
    for e in _edges(lambda r: _tier(rows, r, 40, 1), 1, 1 << 24):
        cases += [(e, 40), (e + 1, 40)]
    return sorted(set(cases))


def _cm_cases():
    cm = _lib().KD_CHANNEL_MAJOR
    cases = [(1, 2, 1), (2, 50, 63), (3, 50, 257), (2, 130, 1025), (2, 50, 2048)]
    for e in _edges(lambda c: _tier(cm, 2, c, 63), 2, 4096):
        cases += [(2, e, 63), (2, e + 1, 63)]
    for e in _edges(lambda n: _tier(cm, 1, 2, n), 1, 1 << 24):
        cases += [(1, 2, e), (1, 2, e + 1)]
    return sorted(set(cases))


ROWS_CASES, CM_CASES = _rows_cases(), _cm_cases()


def test_the_query_reports_edges_in_both_directions():
    """Both layouts have a class edge and a row edge, and the case lists reach every tier on both sides of them."""
    L = _lib()
    assert {_tier(L.KD_ROWS, r, c, 1) for r, c in ROWS_CASES} == {0, 1, 2, 3}
    assert {_tier(L.KD_CHANNEL_MAJOR, b, c, n) for b, c, n in CM_CASES} >= {0, 1, 2}


@functools.lru_cache(maxsize=None)
def _inputs(R, Cn):
    s = 0
    for ch in repr(("kd", R, Cn)):
        s = (s * 131 + ord(ch)) % 2147483629
    g = torch.Generator().manual_seed(s)
    return K.make_logits(g, R, Cn, 0), K.make_logits(g, R, Cn, 1), K.make_targets(g, R, Cn)


@functools.lru_cache(maxsize=None)
def _reference(R, Cn, params):
    s, t, y = _inputs(R, Cn)
    T, alpha, eps = params
    return K.kd_reference(s, t, y, T, alpha, eps, upstream=UPSTREAM)       # (read-only: shared between the tests)


def check(got, ref, name=""):
    """{L, CE, KL} within OUT_RTOL of max(|reference|, 1), dlogits within GRAD_RTOL of the reference tensor's max; all finite."""
    assert np.isfinite(got["out0"]).all() and np.isfinite(got["dx0"]).all(), name
    assert got["dx0"].shape == ref["dx0"].shape, (name, got["dx0"].shape, ref["dx0"].shape)
    e_out = np.abs(np.asarray(got["out0"], dtype=np.float64) - ref["out0"]) / np.maximum(np.abs(ref["out0"]), 1.0)
    scale = max(float(np.abs(ref["dx0"]).max()), 1e-30)
    e_grad = float(np.abs(got["dx0"].astype(np.float64) - ref["dx0"]).max()) / scale
    print("%s: {L,CE,KL} rel err %s, dlogits rel err %.3e" % (name, e_out, e_grad))
    assert (e_out <= OUT_RTOL).all(), "%s: {L,CE,KL} %r vs %r (rel err %r)" % (name, got["out0"], ref["out0"], e_out)
    assert e_grad <= GRAD_RTOL, "%s: dlogits rel err %.3e > %.1e" % (name, e_grad, GRAD_RTOL)
    return float(e_out.max()), e_grad


def run_kd(layout_fn, s, t, y, params, dev):
    T, alpha, eps = params
    sd = s.to(dev).requires_grad_(True)
    loss, parts = layout_fn(sd, t.to(dev), y.to(dev), T=T, alpha=alpha, smoothing=eps > 0, return_parts=True)
    loss.backward(torch.tensor(UPSTREAM, device=dev))
    parts = parts.cpu().numpy()
    assert float(loss.detach()) == float(parts[0])
    return {"out0": parts.astype(np.float64), "dx0": sd.grad.cpu().numpy()}


@pytest.mark.parametrize("params", PARAMS, ids=PARAM_IDS)
@pytest.mark.parametrize("case", ROWS_CASES, ids=["R%d_C%d" % c for c in ROWS_CASES])
def test_rows_kernel_matches_float64(case, params, hip_device):
    from svnet_amd.train import kd_loss
    s, t, y = _inputs(*case)
    if case == (4097, 40) and params[0] <= 1.0:
        assert float(torch.softmax(t / params[0], 1).min()) == 0.0          # teacher probabilities that underflow to 0 in fp32 do occur
    check(run_kd(kd_loss, s, t, y, params, hip_device), _reference(*case, params), "kd rows %r %r" % (case, params))


@pytest.mark.parametrize("params", PARAMS, ids=PARAM_IDS)
@pytest.mark.parametrize("case", CM_CASES, ids=["B%d_C%d_N%d" % c for c in CM_CASES])
def test_channel_major_kernel_matches_float64_and_the_rows_kernel(case, params, hip_device):
    from svnet_amd.train import kd_loss, kd_seg_loss
    B, Cn, N = case
    s, t, y = _inputs(B * N, Cn)
    ref = _reference(B * N, Cn, params)
    ref_cm = {"out0": ref["out0"], "dx0": K.channel_major(torch.from_numpy(ref["dx0"]), B, N).numpy()}
    got = run_kd(kd_seg_loss, K.channel_major(s, B, N), K.channel_major(t, B, N), y.view(B, N), params, hip_device)
    check(got, ref_cm, "kd channel-major %r %r" % (case, params))
    # ... and the rows kernel on the transposed copy of the same data, to the same tolerances
    rows = run_kd(kd_loss, s, t, y, params, hip_device)
    check(got, {"out0": rows["out0"], "dx0": K.channel_major(torch.from_numpy(rows["dx0"]), B, N).numpy().astype(np.float64)},
          "kd channel-major vs rows kernel %r %r" % (case, params))


@pytest.mark.parametrize("case", [(7, 65), (4097, 40), (33, 2)], ids=lambda c: "R%d_C%d" % c)
@pytest.mark.parametrize("smoothing", [True, False])
def test_alpha_zero_is_cal_loss(case, smoothing, hip_device):
    """Rows layout, alpha = 0: dlogits equal SmoothCE's bit for bit (+-0 compare equal: the KD half adds 0 * finite), whatever the teacher;
    the loss equals cal_loss's within OUT_RTOL.  (Both are instantiations of one kernel template, smooth_ce_kernel<KD> (csrc/loss.hip),
    and the cross entropy's operations are smooth_ce.h's in both: the gradient's are single-rounded and identical.  The loss's fused
    multiply-adds remain the compiler's choice per instantiation, so the loss is not asserted bitwise.)"""
    from svnet_amd.train import cal_loss, kd_loss
    s, t, y = _inputs(*case)
    a, b = s.to(hip_device).requires_grad_(True), s.to(hip_device).requires_grad_(True)
    l_kd = kd_loss(a, t.to(hip_device), y.to(hip_device), T=4.0, alpha=0.0, smoothing=smoothing)
    l_ce = cal_loss(b, y.to(hip_device), smoothing=smoothing)
    up = torch.tensor(UPSTREAM, device=hip_device)
    l_kd.backward(up)
    l_ce.backward(up)
    assert np.array_equal(a.grad.cpu().numpy(), b.grad.cpu().numpy())
    l_kd, l_ce = float(l_kd.detach()), float(l_ce.detach())
    assert abs(l_kd - l_ce) <= OUT_RTOL * max(1.0, abs(l_ce)), (l_kd, l_ce)


@pytest.mark.parametrize("layout", ["rows", "channel_major"])
def test_two_launches_are_bit_identical(layout, hip_device):
    from svnet_amd.train import kd_loss, kd_seg_loss
    B, Cn, N = 3, 50, 1500                       # 4500 rows: the rows kernel strides, every workgroup adds partials
    s, t, y = _inputs(B * N, Cn)
    if layout == "rows":
        fn, args = kd_loss, (s, t, y)
    else:
        fn, args = kd_seg_loss, (K.channel_major(s, B, N), K.channel_major(t, B, N), y.view(B, N))
    a, b = (run_kd(fn, *args, PARAMS[1], hip_device) for _ in range(2))
    assert np.array_equal(a["out0"], b["out0"]) and np.array_equal(a["dx0"], b["dx0"])
    assert a["out0"][1] > 0 and a["out0"][2] > 0


def test_the_comparison_can_fail(hip_device):
    """One reference dlogits element off by one part in 1e3 fails check(); an untouched copy passes."""
    from svnet_amd.train import kd_loss
    case, params = (7, 65), PARAMS[1]
    got = run_kd(kd_loss, *_inputs(*case), params, hip_device)
    ref = _reference(*case, params)
    check(got, ref, "teeth: untouched")
    bad = {"out0": ref["out0"], "dx0": ref["dx0"].copy()}
    i = int(np.abs(bad["dx0"]).argmax())
    bad["dx0"].flat[i] *= 1.0 + 1e-3
    with pytest.raises(AssertionError):
        check(got, bad, "teeth: one element off")
    bad = {"out0": ref["out0"] * np.array([1.0, 1.0, 1.0 + 1e-3]), "dx0": ref["dx0"]}
    with pytest.raises(AssertionError):
        check(got, bad, "teeth: KL off")


@pytest.mark.parametrize("layout", ["rows", "channel_major"])
def test_a_teacher_equal_to_the_student_teaches_nothing(layout, hip_device):
    from svnet_amd.train import kd_loss, kd_seg_loss
    B, Cn, N = 2, 50, 257
    s, _, y = _inputs(B * N, Cn)
    R = B * N
    if layout == "rows":
        fn, args = kd_loss, (s, s.clone(), y)
    else:
        fn, args = kd_seg_loss, (K.channel_major(s, B, N), K.channel_major(s, B, N), y.view(B, N))
    sd = args[0].to(hip_device).requires_grad_(True)
    loss, parts = fn(sd, args[1].to(hip_device), args[2].to(hip_device), T=4.0, alpha=1.0, return_parts=True)
    loss.backward()
    parts = parts.cpu().numpy()
    print("teacher == student: parts %r, max |dlogits| %.3e" % (parts, float(sd.grad.abs().max())))
    assert np.isfinite(parts).all() and abs(float(parts[2])) <= 1e-6
    assert float(sd.grad.abs().max()) <= GRAD_RTOL / R


def test_unsupported_shapes_and_wrong_devices_raise(hip_device):
    from svnet_amd._lib import SvnetHipError
    from svnet_amd.train import kd_loss, kd_seg_loss
    z = torch.zeros(4, 1, device=hip_device)
    with pytest.raises(SvnetHipError, match="not supported"):
        kd_loss(z, z, torch.zeros(4, dtype=torch.int64, device=hip_device))
    z3 = torch.zeros(2, 1, 8, device=hip_device)
    with pytest.raises(SvnetHipError, match="not supported"):
        kd_seg_loss(z3, z3, torch.zeros(2, 8, dtype=torch.int64, device=hip_device))
    s = torch.zeros(4, 40, device=hip_device)
    with pytest.raises(ValueError, match="teacher on cpu"):
        kd_loss(s, torch.zeros(4, 40), torch.zeros(4, dtype=torch.int64, device=hip_device))


# ----------------------------------------------------------------------------- a teacher beside the student

def _case(tag):
    return [c for c in TRAIN_CASES if c[0] == tag][0]


def _pair(tag_student, dev, students=1):
    """The binary student(s) of a TRAIN_CASES case and a full-precision teacher of the same model and shape, on the case's own batch."""
    from oracle import params as oparams
    tag, model, binary, B, N, k = _case(tag_student)
    assert binary
    P = oparams.synthetic_params(model, binary=True, seed=C.SEED)
    studs = [build_model(model, True, k, dev, P).train() for _ in range(students)]
    teacher = build_model(model, False, k, dev, oparams.synthetic_params(model, binary=False, seed=C.SEED))
    x, l, y = C.model_inputs(tag, model, B, N)
    inputs = (x.to(dev),) if l is None else (x.to(dev), l.to(dev))
    return studs, teacher, inputs, y.to(dev)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-30)


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_alpha_zero_distilled_step_is_the_plain_step(captured, hip_device):
    """A Distiller with alpha = 0 changes nothing about the student's step: same loss, same flat gradient bucket as the plain cal_loss
    step on the same weights and batch - eager and captured, twice in a row without an optimizer step.  Teacher and student share the
    packed-weight cache, the zero arena and the k-NN table: state of the other model left in any of them is a gross mismatch."""
    from svnet_amd.train import Distiller, TrainStep
    (plain_m, kd_m), teacher, inputs, y = _pair("dgcnn_bin_small", hip_device, students=2)
    plain = TrainStep(plain_m, inputs, y)
    want_loss = float(plain.fwd_bwd())
    want = plain.bucket.flat.clone()
    scale = float(want.abs().max())
    assert np.isfinite(scale) and scale > 0
    d = Distiller(teacher, inputs, T=4.0, alpha=0.0)
    if captured:
        d.capture()
    d.run()
    step = TrainStep(kd_m, inputs, y, loss_fn=d.loss_fn)
    if captured:
        step.capture()
    for r in range(2):
        d.run()
        loss = float(step.run(all_reduce=False))
        err = float((step.bucket.flat - want).abs().max()) / scale
        print("run %d: loss %r vs %r, bucket rel err %.3e" % (r, loss, want_loss, err))
        assert abs(loss - want_loss) <= OUT_RTOL * max(1.0, abs(want_loss)), (r, loss, want_loss)
        assert err <= GRAD_RTOL, "run %d: bucket differs from the plain step by %.3e of its max" % (r, err)
    assert float(d.parts[2]) > 0 and not teacher.training and kd_m.training


def test_teacher_logits_survive_the_students_optimizer_step(hip_device):
    from svnet_amd.train import Distiller, FlatAdam, FlatParams, TrainStep
    (student,), teacher, inputs, y = _pair("dgcnn_bin_small", hip_device)
    fp = FlatParams(student)
    d = Distiller(teacher, inputs, T=4.0, alpha=0.5).capture()
    before = d.run().clone()
    step = TrainStep(student, inputs, y, loss_fn=d.loss_fn, keep_output=True).capture()
    opt = FlatAdam(fp, step.bucket, lr=1e-2)
    d.run()
    step.run(all_reduce=False)
    s_before = step.out.clone()
    opt.step()
    after = d.run().clone()
    step.run(all_reduce=False)
    print("teacher moved %.3e, student moved %.3e" % (_rel(after, before), _rel(step.out, s_before)))
    assert _rel(after, before) <= OUT_RTOL
    assert _rel(step.out, s_before) > 1e-3


def test_step_gradient_is_the_reference_on_the_steps_own_logits(hip_device):
    from svnet_amd.train import Distiller, TrainStep
    (student,), teacher, inputs, y = _pair("dgcnn_bin_small", hip_device)
    d = Distiller(teacher, inputs, T=4.0, alpha=0.5)
    seen = []

    def loss_fn(out, target):
        out.register_hook(lambda g: seen.append(g.clone()))
        return d.loss_fn(out, target)
    step = TrainStep(student, inputs, y, loss_fn=loss_fn, keep_output=True)
    d.run()
    loss = float(step.run(all_reduce=False))
    ref = K.kd_reference(step.out.cpu(), d.logits.cpu(), y.cpu(), 4.0, 0.5, 0.2)
    got = {"out0": d.parts.cpu().numpy().astype(np.float64), "dx0": seen[-1].cpu().numpy()}
    assert loss == float(got["out0"][0]) and len(seen) == 1
    check(got, ref, "distilled step, alpha 0.5")
    assert float(ref["out0"][2]) > 1e-3                                  # (the teacher does differ from the student)


def test_captured_student_over_an_eager_teacher(hip_device):
    """The loss reads the teacher's logits at a fixed address: a captured student step sees what an eager teacher computed for THIS batch."""
    from svnet_amd.train import Distiller, TrainStep
    (s_a, s_b), teacher, inputs, y = _pair("dgcnn_bin_small", hip_device, students=2)
    losses = {}
    for key, student in (("eager", s_a), ("captured", s_b)):
        inputs[0].mul_(-1.0)                                             # capture on one batch ...
        d = Distiller(teacher, inputs, T=4.0, alpha=0.5)
        if key == "captured":
            d.capture()
        d.run()
        addr = d.logits.data_ptr()
        step = TrainStep(student, inputs, y, loss_fn=d.loss_fn).capture()
        inputs[0].mul_(-1.0)                                             # ... replay on another
        d.run()
        losses[key] = float(step.run(all_reduce=False))
        assert d.logits.data_ptr() == addr
        stale = float(step.run(all_reduce=False))                        # (no teacher run in between: same logits, same loss)
        assert stale == losses[key]
    print("captured student: loss over eager teacher %r, over captured teacher %r" % (losses["eager"], losses["captured"]))
    assert abs(losses["eager"] - losses["captured"]) <= OUT_RTOL * max(1.0, abs(losses["captured"])), losses


def test_train_epoch_with_a_teacher(hip_device):
    from oracle import params as oparams
    from svnet_amd.data import BatchLoader, DevicePool
    from svnet_amd.train import Distiller, FlatAdam, FlatParams, TrainStep, train_epoch
    pool = DevicePool.synthetic(5, 24, 64, 40, device=hip_device)
    teacher = build_model("sv_dgcnn_cls", False, 8, hip_device, oparams.synthetic_params("sv_dgcnn_cls", binary=False, seed=C.SEED))
    P = oparams.synthetic_params("sv_dgcnn_cls", binary=True, seed=C.SEED)

    def run(alpha):
        student = build_model("sv_dgcnn_cls", True, 8, hip_device, P).train()
        fp = FlatParams(student)
        loader = BatchLoader(pool, 4, 64, select="first_shuffled", scale_shift=True, rotate="none", seed=9)
        d = None if alpha is None else Distiller(teacher, (loader.x,), T=4.0, alpha=alpha)
        step = TrainStep(student, (loader.x,), loader.y, **({} if d is None else {"loss_fn": d.loss_fn}))
        opt = FlatAdam(fp, step.bucket, lr=1e-3)
        losses = []

        class Spy:
            def run(self):
                loss = step.run()
                losses.append(loss.detach().clone())
                return loss
        means = []
        for epoch in range(2):
            loader.set_epoch(epoch)
            means.append(train_epoch(Spy(), loader, opt, teacher=d))
        assert len(losses) == 12 and opt.steps == 12
        return means, float(losses[0])
    plain, first_plain = run(None)
    kd, _ = run(0.5)
    _, first_zero = run(0.0)
    print("mean losses: plain %r, distilled %r; first step plain %r, alpha 0 %r" % (plain, kd, first_plain, first_zero))
    assert all(np.isfinite(plain)) and all(np.isfinite(kd))
    assert all(abs(a - b) > 1e-3 for a, b in zip(plain, kd))
    assert abs(first_zero - first_plain) <= OUT_RTOL * max(1.0, abs(first_plain))


def test_part_segmentation_step_captures_and_replays(hip_device):
    """sv_dgcnn_partseg, binary student and full-precision teacher, kd_seg_loss on the [B,num_part,N] logits where they lie: captured,
    replayed, and the gradient that reaches the student's logits is the float64 reference on the step's own logits."""
    from svnet_amd.train import Distiller, TrainStep
    (student,), teacher, inputs, y = _pair("pseg_bin_small", hip_device)
    d = Distiller(teacher, inputs, T=4.0, alpha=0.5, seg=True)      # (an eager teacher: the student's captured step reads its fixed buffer)
    held = []

    def loss_fn(out, target):
        out.register_hook(lambda g: held.append(g))          # (kept alive through the capture: its buffer is not reused inside the graph)
        return d.loss_fn(out, target)
    d.run()
    step = TrainStep(student, inputs, y, loss_fn=loss_fn, keep_output=True).capture()
    for _ in range(2):
        d.run()
        loss = float(step.run(all_reduce=False))
    assert step.out.dim() == 3 and step.out.shape[1] == 50 and tuple(held[-1].shape) == tuple(step.out.shape)
    ref = K.kd_reference(step.out.cpu(), d.logits.cpu(), y.cpu(), 4.0, 0.5, 0.2)
    got = {"out0": d.parts.cpu().numpy().astype(np.float64), "dx0": held[-1].cpu().numpy()}
    assert loss == float(got["out0"][0])
    check(got, ref, "part-seg distilled step")
    assert torch.isfinite(step.bucket.flat).all() and float(step.bucket.flat.abs().max()) > 0
