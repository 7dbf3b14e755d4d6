"""CPU: the host side of losses.SoftmaxLoss and evaluation.LabelAccuracyEvaluator -- the classifier's shape per flag
combination, constructor defaults, state_dict keys, the layout of loss_params.LossParameters (256-element chunks, decay flags,
zero padding, views that survive .to() / .float() / load_state_dict), the drop-in namespaces and the library's exports
against the header. No kernel runs here: where the class computes, it is its torch path on CPU tensors."""
import inspect
import os
import sys

import pytest
import torch
from torch import nn

import quadruplet_sentence_transformer_amd  # noqa: F401
import softmax_head_helpers as SH
from quadruplet_sentence_transformer_amd import _lib, evaluation, st_losses as S
from quadruplet_sentence_transformer_amd.loss_params import CHUNK, LossParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = inspect.Parameter.empty


def defaults(fn, skip=("self",)):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if k not in skip}


# ------------------------------------------------------------------ surface
def test_constructor_defaults_follow_sentence_transformers():
    d = defaults(S.SoftmaxLoss.__init__)
    assert isinstance(d.pop("loss_fct"), nn.CrossEntropyLoss)
    assert d == {"model": EMPTY, "sentence_embedding_dimension": EMPTY, "num_labels": EMPTY, "concatenation_sent_rep": True,
                 "concatenation_sent_difference": True, "concatenation_sent_multiplication": False, "fused": True}
    assert list(defaults(S.SoftmaxLoss.__init__))[:7] == [
        "model", "sentence_embedding_dimension", "num_labels", "concatenation_sent_rep", "concatenation_sent_difference",
        "concatenation_sent_multiplication", "loss_fct"]
    assert list(inspect.signature(S.SoftmaxLoss.forward).parameters) == ["self", "sentence_features", "labels"]
    assert defaults(evaluation.LabelAccuracyEvaluator.__init__) == {"dataloader": EMPTY, "name": "", "softmax_model": None,
                                                                    "write_csv": True}
    assert issubclass(evaluation.LabelAccuracyEvaluator, evaluation.SentenceEvaluator)
    assert defaults(evaluation.LabelAccuracyEvaluator.__call__) == {"model": EMPTY, "output_path": None, "epoch": -1, "steps": -1}
    ev = evaluation.LabelAccuracyEvaluator([], name="dev")
    assert ev.csv_file == "accuracy_evaluation_dev_results.csv" and ev.csv_headers == ["epoch", "steps", "accuracy"]
    assert evaluation.LabelAccuracyEvaluator([]).csv_file == "accuracy_evaluation_results.csv"
    assert S.SoftmaxLoss(nn.Identity(), 8, 2).reduction == "mean"


@pytest.mark.parametrize("flags,nvec,parts", [((True, True, False), 3, 3), ((True, True, True), 4, 7), ((True, False, False), 2, 1),
                                              ((False, True, False), 1, 2), ((False, False, True), 1, 4),
                                              ((False, True, True), 2, 6), ((True, False, True), 3, 5)])
def test_classifier_shape_and_initial_weights_per_flag_combination(flags, nvec, parts):
    D, C = 64, 3
    torch.manual_seed(123)
    lm = S.SoftmaxLoss(nn.Identity(), D, C, *flags)
    torch.manual_seed(123)
    ref = nn.Linear(nvec * D, C)             # what sentence-transformers builds from the same seed
    assert isinstance(lm.classifier, nn.Linear)
    assert lm.classifier.weight.shape == (C, nvec * D) and lm.classifier.bias.shape == (C,)
    assert torch.equal(lm.classifier.weight, ref.weight) and torch.equal(lm.classifier.bias, ref.bias)
    assert lm._parts == parts and SH.nvec(parts) == nvec and lm.num_labels == C
    # the torch path of the class (CPU tensors) is the 2.2.2 definition
    u, v, _, _, labels = SH.case(5, D, C, parts, 1)
    lm._embed = lambda feats, k: [u, v]
    want = SH.loss_ref(u, v, ref.weight, ref.bias, labels, parts)
    assert torch.allclose(lm(None, labels), want)
    reps, logits = lm(None, None)
    assert reps[0] is u and reps[1] is v and torch.allclose(logits, SH.logits_ref(u, v, ref.weight, ref.bias, parts))


def test_no_part_selected_is_refused():
    with pytest.raises(ValueError):
        S.SoftmaxLoss(nn.Identity(), 8, 2, False, False, False)


def test_only_a_default_cross_entropy_takes_the_fused_path():
    mk = lambda f: S.SoftmaxLoss(nn.Identity(), 8, 2, loss_fct=f)._default_ce()  # noqa: E731
    assert mk(nn.CrossEntropyLoss()) and mk(nn.CrossEntropyLoss(ignore_index=1))
    assert not mk(nn.CrossEntropyLoss(reduction="sum")) and not mk(nn.CrossEntropyLoss(weight=torch.ones(2)))
    assert not mk(nn.CrossEntropyLoss(label_smoothing=0.1)) and not mk(nn.MSELoss())
    assert S.softmax_head_supported(64, 3, 3) and S.softmax_head_supported(2048, 8, 7) and S.softmax_head_supported(4, 1, 1)
    assert not S.softmax_head_supported(2052, 3, 3) and not S.softmax_head_supported(64, 9, 3)
    assert not S.softmax_head_supported(66, 3, 3) and not S.softmax_head_supported(64, 3, 0)


def test_state_dict_is_plain_module_behaviour():
    lm = S.SoftmaxLoss(nn.Identity(), 64, 3)
    sd = lm.state_dict()
    assert list(sd) == ["classifier.weight", "classifier.bias"]
    assert [n for n, _ in lm.named_parameters()] == ["classifier.weight", "classifier.bias"]
    new = {"classifier.weight": torch.full((3, 192), 0.25), "classifier.bias": torch.tensor([1.0, 2.0, 3.0])}
    lm.load_state_dict(new)
    op = lm.owned_parameters()
    assert isinstance(op, LossParameters)
    # loaded in place: the flat buffer holds the new values, the padding is still zero
    assert (op.params[:576] == 0.25).all() and (op.params[576:768] == 0).all()
    assert op.params[768:771].tolist() == [1.0, 2.0, 3.0] and (op.params[771:] == 0).all()
    other = S.SoftmaxLoss(nn.Identity(), 64, 3)
    other.load_state_dict(lm.state_dict())
    assert torch.equal(other.classifier.weight, lm.classifier.weight)


# ------------------------------------------------------------------ LossParameters
def inside(t, buf):
    return buf.data_ptr() <= t.data_ptr() and t.data_ptr() + t.numel() * 4 <= buf.data_ptr() + buf.numel() * 4


def test_loss_parameters_layout():
    torch.manual_seed(0)
    mod = nn.Sequential(nn.Linear(300, 3), nn.Linear(3, 2, bias=False))
    want = {n: p.detach().clone() for n, p in mod.named_parameters()}
    op = LossParameters(mod)
    assert CHUNK == 256
    # every tensor starts on a chunk and is padded to whole chunks: 900 -> 1024, 3 -> 256, 6 -> 256
    assert [(n, o, k, d) for n, o, k, _, d in op.layout] == [("0.weight", 0, 900, True), ("0.bias", 1024, 3, False),
                                                            ("1.weight", 1280, 6, True)]
    assert op.total == 1536 and op.params.shape == op.grads.shape == (1536,) and op.params.dtype == torch.float32
    # one decay flag per chunk; names ending in `bias` do not decay (sentence-transformers' no_decay filter)
    assert op.chunk_decay.dtype == torch.uint8 and op.chunk_decay.tolist() == [1, 1, 1, 1, 0, 1]
    for n, o, k, shape, _ in op.layout:
        p = dict(mod.named_parameters())[n]
        assert torch.equal(p, want[n]) and p.data_ptr() == op.params.data_ptr() + 4 * o
        assert p.grad is not None and p.grad.data_ptr() == op.grads.data_ptr() + 4 * o and p.grad.shape == p.shape
        assert torch.equal(op.params[o:o + k].view(shape), want[n])
        assert int(torch.count_nonzero(op.params[o + k:(o + k + CHUNK - 1) // CHUNK * CHUNK])) == 0      # the padding
    assert int(torch.count_nonzero(op.grads)) == 0
    # the moments come with the first step that asks for them
    assert op.exp_avg is None and op.exp_avg_sq is None
    op.ensure_state()
    assert op.exp_avg.shape == op.exp_avg_sq.shape == (1536,) and int(torch.count_nonzero(op.exp_avg)) == 0
    with pytest.raises(ValueError):
        LossParameters(nn.Identity())


def test_autograd_accumulates_into_the_flat_gradient_buffer():
    lin = nn.Linear(5, 2)
    op = LossParameters(lin)
    x = torch.randn(4, 5)
    lin(x).sum().backward()
    lin(x).sum().backward()
    assert lin.weight.grad.data_ptr() == op.grads.data_ptr()
    assert torch.allclose(op.grads[:10].view(2, 5), 2 * x.sum(0).expand(2, 5)) and torch.allclose(op.grads[256:258], torch.full((2,), 8.0))
    op.zero_grad()
    assert int(torch.count_nonzero(lin.weight.grad)) == 0 and int(torch.count_nonzero(lin.bias.grad)) == 0


def test_ensure_rebuilds_the_views_after_the_module_was_converted():
    lin = nn.Linear(5, 2)
    op = LossParameters(lin)
    want = lin.weight.detach().clone()
    lin.double()                                  # nn.Module._apply replaces .data: the parameters leave the buffer
    assert not inside(lin.weight, op.params)
    with torch.no_grad():
        lin.weight.mul_(2.0)                      # ... and may change before anybody looks again
    assert op.ensure() is op
    assert lin.weight.dtype == torch.float32 and inside(lin.weight, op.params) and inside(lin.bias, op.params)
    assert inside(lin.weight.grad, op.grads) and inside(lin.bias.grad, op.grads)
    assert torch.equal(lin.weight, 2.0 * want) and torch.equal(op.params[:10].view(2, 5), 2.0 * want)
    # a dropped .grad (zero_grad(set_to_none=True)) is bound again; one that autograd replaced is copied in
    lin.zero_grad(set_to_none=True)
    assert lin.weight.grad is None
    lin(torch.ones(1, 5)).sum().backward()
    assert not inside(lin.weight.grad, op.grads)
    op.ensure()
    assert inside(lin.weight.grad, op.grads) and (op.grads[:10] == 1.0).all() and (op.grads[256:258] == 1.0).all()
    ptrs = [p.data_ptr() for p in lin.parameters()]
    op.ensure()                                   # nothing to do: nothing moves
    assert ptrs == [p.data_ptr() for p in lin.parameters()]


def test_softmax_loss_keeps_its_parameters_in_the_buffer_across_to_and_forward():
    lm = S.SoftmaxLoss(nn.Identity(), 8, 2)
    op = lm.owned_parameters()
    lm.to("cpu")
    lm.double()
    u, v = torch.randn(3, 8), torch.randn(3, 8)
    lm._embed = lambda feats, k: [u, v]
    lm(None, torch.tensor([0, 1, 1])).backward()  # forward calls ensure() first
    assert inside(lm.classifier.weight, op.params) and inside(lm.classifier.bias, op.params)
    assert inside(lm.classifier.weight.grad, op.grads) and op.grads[:24].abs().max().item() > 0


# ------------------------------------------------------------------ namespaces and exports
def test_dropin_names_resolve_to_this_build():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]
        from sentence_transformers import evaluation as ev, losses
        assert losses.SoftmaxLoss is S.SoftmaxLoss
        assert ev.LabelAccuracyEvaluator is evaluation.LabelAccuracyEvaluator
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]


def test_library_exports_the_new_entry_points():
    lib = _lib.load()
    assert lib.qst_version() >= 108
    names = ["qst_clip_adamw_step_joint", "qst_softmax_head_fwd", "qst_softmax_head_bwd", "qst_softmax_head_bwd_workspace_bytes",
             "qst_softmax_ce"]
    header = open(os.path.join(ROOT, "include", "qst.h")).read()
    for name in names:                            # (tests/test_abi_layout.py holds the table to the headers as a whole)
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["qst_clip_adamw_step_joint"][1]) == 22
    assert len(_lib.SIGNATURES["qst_softmax_head_fwd"][1]) == 10 and len(_lib.SIGNATURES["qst_softmax_head_bwd"][1]) == 15
    assert len(_lib.SIGNATURES["qst_softmax_ce"][1]) == 12
    # size query and argument checks need no device
    assert lib.qst_softmax_head_bwd_workspace_bytes(64, 64, 3, 3) == 0
    assert lib.qst_softmax_head_bwd_workspace_bytes(257, 64, 3, 3) == 5 * 3 * (3 * 64 + 4) * 4
    assert lib.qst_softmax_head_bwd_workspace_bytes(10 ** 6, 64, 3, 3) == 32 * 3 * (3 * 64 + 4) * 4
    assert lib.qst_softmax_head_bwd_workspace_bytes(257, 64, 3, 0) == 0
    assert lib.qst_softmax_head_fwd(None, None, None, None, 1, 4, 1, 1, None, None) == SH.BAD_ARG
    assert lib.qst_softmax_ce(None, None, 1, 1, -100, 2, None, None, None, None, None, None) == SH.BAD_ARG
    assert lib.qst_clip_adamw_step_joint(*([None] * 10), 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1, None, None, None) == SH.BAD_ARG
