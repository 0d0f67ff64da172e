"""CPU tests: the oracle (oracle/) against the golden vectors captured from the imported reference
(tests/golden/make_golden.py)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import knn as oknn
from oracle import params as oparams
from oracle import sv_ref
from tests.common import GOLDEN, compare_case, load_npz
from tests.golden import cases as C
from tests.golden import harness as H


@pytest.mark.parametrize("case", C.KNN_CASES, ids=[c[0] for c in C.KNN_CASES])
def test_knn_exact_matches_reference_indices(case):
    name, B, N, Cc, k, layout = case
    x = C.knn_input(*case)
    idx, pd = oknn.knn_exact(x, k, return_pd=True)
    ref = torch.from_numpy(load_npz("knn.npz")[name].astype(np.int64))
    assert oknn.tie_aware_mismatches(ref, idx, pd) == 0
    assert (idx[..., 0] == torch.arange(N).view(1, N)).all()          # self is the nearest neighbour


def test_knn_torch_chain_agrees_with_exact_here():
    x = C.knn_input(*C.KNN_CASES[1])
    a = oknn.knn_torch(x, 20)
    b, pd = oknn.knn_exact(x, 20, return_pd=True)
    assert oknn.tie_aware_mismatches(a, b, pd) == 0


def test_knn_rejects_unsupported():
    with pytest.raises(ValueError):
        oknn.knn_exact(torch.zeros(1, 400, 8), 2)                      # C > 384: outside the bit-exact contract


_OPS = H.op_cases()


@pytest.mark.parametrize("name", list(_OPS), ids=list(_OPS))
def test_oracle_ops_match_golden(name):
    gold = load_npz("ops.npz")
    ref = {k.split("/", 1)[1]: gold[k] for k in gold.files if k.startswith(name + "/")}
    assert ref, name
    got = H.to_numpy(_OPS[name](H.OracleAPI()))
    assert set(got) == set(ref)
    compare_case(got, ref, 2e-5, name)


def _oracle_forward(model, x, l, P, k, binary, ctx):
    if model == "sv_dgcnn_cls":
        return sv_ref.sv_dgcnn_cls(x, P, k, binary, ctx)
    if model == "sv_pointnet_cls":
        return sv_ref.sv_pointnet_cls(x, P, k, binary, ctx)
    if model == "sv_pointnet_pseg":
        return sv_ref.sv_pointnet_pseg(x, l, P, k, binary, ctx)
    return sv_ref.sv_dgcnn_pseg(x, l, P, k, binary, ctx)


@pytest.mark.parametrize("case", C.MODEL_CASES, ids=[c[0] for c in C.MODEL_CASES])
def test_oracle_models_match_golden(case):
    tag, model, binary, B, N, k = case
    gold = load_npz("models.npz")
    x, l, y = C.model_inputs(tag, model, B, N)
    P = oparams.synthetic_params(model, binary=binary, seed=C.SEED)
    with torch.no_grad():
        ev = _oracle_forward(model, x, l, P, k, binary, sv_ref.Ctx(train=False)).numpy()
    assert H.max_rel_err(ev, gold[tag + "/logits_eval"]) < 1e-5
    chaotic = float(gold[tag + "/self_sensitivity"]) > 1e-2
    if model == "sv_pointnet_pseg" and binary:
        # the REFERENCE's own train-mode forward moves by O(1) when its input is scaled by (1 + 1e-7) (make_golden.py measures it:
        # sv_pointnet_partseg --binary): train mode of this case cannot be pinned element-wise by anything; eval mode (above) is
        assert chaotic
        return
    Pg = oparams.synthetic_params(model, binary=binary, seed=C.SEED, requires_grad=True)
    ctx = sv_ref.Ctx(train=True, collect_bn=True)
    lo = _oracle_forward(model, x, l, Pg, k, binary, ctx)
    # per-cloud BN over B=4 rows (PointNet STN, fp) amplifies rounding: 1e-3 there, 1e-5 elsewhere
    tol = 2e-3 if (model in ("sv_pointnet_cls", "sv_pointnet_pseg") and not binary) else 1e-5
    if chaotic and (tag + "/logits_train" not in gold.files or H.max_rel_err(lo.detach().numpy(), gold[tag + "/logits_train"]) >= tol):
        # a case whose reference moves by more than 1e-2 under the 1e-7 input scaling (BatchNorm over B = 2 rows: dgcnn_bin_full,
        # pseg_bin_full) is reproduced in train mode only by luck of the same BLAS: pinned by its eval logits
        return
    assert H.max_rel_err(lo.detach().numpy(), gold[tag + "/logits_train"]) < tol
    if l is not None:
        loss = sv_ref.cal_loss(lo.permute(0, 2, 1).reshape(-1, lo.shape[1]), y.reshape(-1))
    else:
        loss = sv_ref.cal_loss(lo, y)
    assert abs(float(loss) - float(gold[tag + "/loss_train"])) < max(tol, 1e-5) * max(1.0, abs(float(loss)))
    loss.backward()
    names = [str(n) for n in gold[tag + "/param_names"]]
    gn = np.array([float(Pg[n].grad.norm()) if Pg[n].grad is not None else 0.0 for n in names])
    ref = gold[tag + "/grad_norms"].astype(np.float64)
    # gradient norms, relative to the largest one (scales feeding a train-mode BN have ~0 gradient = noise)
    # Binary PointNet max-pools discrete-valued scalars over the N points: candidates with the same integer
    # popcount tie, and in the reference's train mode the tie is broken by the 1e-7 noise of its
    # (sign(x)+x)-x STE arithmetic, so WHICH point receives the gradient is not reproducible.
    gtol = 0.1 if (model in ("sv_pointnet_cls", "sv_pointnet_pseg") and binary) else max(tol * 10, 1e-4)
    assert np.abs(gn - ref).max() / ref.max() < gtol
    bn_key = "conv2.bn1" if "conv2.bn1.running_mean" in P else "feat.conv1.bn1"
    assert H.max_rel_err(ctx.bn_updates[bn_key + ".running_mean"].numpy(), gold[tag + "/bn_running_mean"]) < 1e-4
    assert H.max_rel_err(ctx.bn_updates[bn_key + ".running_var"].numpy(), gold[tag + "/bn_running_var"]) < 1e-4


def test_state_layouts_agree():
    """reference state_dict layout (golden) == oracle spec == product modules, key for key."""
    import argparse
    import contextlib
    import io
    import svnet_amd.models as M
    layout = json.load(open(os.path.join(GOLDEN, "state_layout.json")))
    classes = {"sv_dgcnn_cls": (M.SV_DGCNN_CLS, 40), "sv_pointnet_cls": (M.SV_PointNet_CLS, 40),
               "sv_dgcnn_pseg": (M.SV_DGCNN_PSEG, 50), "sv_pointnet_pseg": (M.SV_PointNet_PSEG, 50)}
    for model, (cls, nc) in classes.items():
        for binary in (True, False):
            ref = [(n, tuple(s)) for n, s in layout["%s/%s" % (model, "binary" if binary else "fp")]]
            kw = {"num_part": nc} if model.endswith("_pseg") else {"num_class": nc}
            spec = oparams.SPECS[model](binary=binary, **kw)
            assert sorted(ref) == sorted((n, tuple(s)) for n, s in spec.items()), model
            with contextlib.redirect_stdout(io.StringIO()):
                m = cls(argparse.Namespace(k=20, binary=binary, dropout=0.5), nc)
            assert ref == [(n, tuple(t.shape)) for n, t in m.state_dict().items()], model


def test_loss_known_answer():
    logits = torch.zeros(3, 40)
    y = torch.tensor([0, 5, 39])
    assert abs(float(sv_ref.cal_loss(logits, y)) - float(np.log(40.0))) < 1e-6     # uniform prediction


def test_rotation_and_permutation_invariance_of_oracle():
    """Known-answer property of the path: logits do not depend on an SO(3) rotation of the
    cloud nor on the order of its points."""
    from svnet_amd import synth
    tag, model, binary, B, N, k = C.MODEL_CASES[0]
    x, _, _ = C.model_inputs(tag, model, B, N)
    P = oparams.synthetic_params(model, binary=False, seed=C.SEED)
    ctx = sv_ref.Ctx(train=False)
    with torch.no_grad():
        base = sv_ref.sv_dgcnn_cls(x, P, k, False, ctx)
        R = torch.from_numpy(synth.random_rotation(7, 3)).float()
        rot = sv_ref.sv_dgcnn_cls(torch.einsum("ij,bjn->bin", R, x), P, k, False, ctx)
        perm = torch.from_numpy(np.random.RandomState(0).permutation(N))
        prm = sv_ref.sv_dgcnn_cls(x[:, :, perm], P, k, False, ctx)
    assert H.max_rel_err(rot.numpy(), base.numpy()) < 1e-4
    assert H.max_rel_err(prm.numpy(), base.numpy()) < 1e-4


def test_oracle_against_recorded_reference_subset():
    """The oracle on the reference's own outputs for a subset of ops, as make_golden.py recorded them from the imported reference
    (tests/golden/ops.npz): the suite needs nothing outside the repository."""
    gold = load_npz("ops.npz")
    api_orc = H.OracleAPI()
    for name in ("gf_sv", "linear_bin_train", "svblock_edge_bin_train", "vector_bn_train", "svpool_k_max"):
        ref = {k.split("/", 1)[1]: gold[k] for k in gold.files if k.startswith(name + "/")}
        got = H.to_numpy(_OPS[name](api_orc))
        assert ref and set(got) == set(ref), name
        compare_case(got, ref, 2e-5, name)


@pytest.mark.parametrize("tag", ["dgcnn_bin_small", "pseg_bin_small"])
def test_exact_ste_mode_differs_from_reference_arithmetic_only_in_tie_breaks(tag):
    """The oracle mode the binary GPU parity tests compare against (Ctx(exact_ste=True)) versus the reference's train-mode
    arithmetic (the oracle's default mode, pinned to the imported reference by the goldens): with the reference-mode arg-max
    selections replayed, every gradient agrees to 1e-4; on its own, the exact mode picks a different element ONLY where the
    candidates tie exactly (and the same k-NN graphs).  The numbers recorded against the imported reference itself by
    make_golden.py are checked too."""
    from tests.golden.make_golden import exact_ste_study
    case = [c for c in C.MODEL_CASES if c[0] == tag][0]
    _, model, _, B, N, k = case
    st = exact_ste_study(tag, model, B, N, k)
    assert st["replay_vs_refmode_grad"] < 1e-4 and st["replay_vs_refmode_logits"] < 1e-5 and st["replay_loss_diff"] < 1e-5, st
    assert st["same_graphs"] and st["selections_differ"] > 0 and st["selections_differ"] == st["differ_and_exact_tie"], st
    assert st["free_vs_refmode_grad"] > 1e-2, "expected visible tie-break differences in this case: %r" % (st,)
    gold = load_npz("models.npz")[tag + "/exact_ste_study"]
    assert gold[0] < 1e-4 and gold[1] < 1e-4 and gold[3] == gold[4] and gold[3] == st["selections_differ"], gold
