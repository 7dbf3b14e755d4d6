"""GPU: models.Dense through the Python surface -- SentenceTransformer loading, encoding, saving, differentiating and fitting
the chain Transformer -> Pooling -> Dense -> [Normalize] on the tiny-bert preset (hidden 64, the synthetic tokenizer).

The yardstick is the TWIN: the same checkpoint directory without the Dense and Normalize entries. What the Dense model returns
is held against the fp64 reference head of dense_head_helpers applied to what the twin returns, and the gradients that reach
the Dense model's encoder against the twin's encoder gradients under the reference's grad_x.
"""
import json
import os

import numpy as np
import pytest
import torch
from torch import nn
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import dense_head_helpers as H  # noqa: E402
from quadruplet_sentence_transformer_amd import models, st_losses as S  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample, SentenceTransformer  # noqa: E402

NOUNS = "cat dog horse bridge river apple street garden window train doctor teacher".split()
VERBS = "sees paints crosses finds leaves follows builds opens".split()
DOUT = 24
TYPES = ["sentence_transformers.models." + k for k in ("Transformer", "Pooling", "Dense", "Normalize")]


def text(i):
    rng = np.random.RandomState(i)
    return " ".join(f"the {rng.choice(NOUNS)} {rng.choice(VERBS)} a {rng.choice(NOUNS)}" for _ in range(1 + i % 3))


SENTENCES = [text(i) for i in range(12)]


def write_pair(tmp_path):
    """The directory with 2_Dense (64 -> 24, tanh) and 3_Normalize, and its twin without them: (dense dir, twin dir, W, b)."""
    w, b = H.write_model_dir(str(tmp_path / "dense"), Dout=DOUT, act=H.TANH)
    H.write_model_dir(str(tmp_path / "twin"), kinds=("Transformer", "Pooling"))
    return str(tmp_path / "dense"), str(tmp_path / "twin"), w, b


def head_of(x, w, b, act=H.TANH, normalize=1):
    """The fp64 reference head on fp32 inputs."""
    return H.head_ref(torch.as_tensor(x).double().cpu(), w.double(), None if b is None else b.double(), act, normalize)[2]


def dense_params(model):
    named = dict(model.named_parameters())
    return named["2.linear.weight"], named.get("2.linear.bias")


# ------------------------------------------------------------------ 1. encode
def test_encode_equals_the_reference_head_on_the_twins_embeddings(tmp_path):
    ddir, tdir, w, b = write_pair(tmp_path)
    model, twin = SentenceTransformer(ddir, device="cuda"), SentenceTransformer(tdir, device="cuda")
    assert model.cfg.normalize is False and twin.cfg.normalize is False and model._dense_normalize is True
    names = [n for n, _ in model.named_parameters()]
    assert "2.linear.weight" in names and "2.linear.bias" in names and any(n.startswith("0.auto_model.") for n in names)
    for precision in (None, "bf16x3"):
        got = model.encode(SENTENCES, batch_size=5, precision=precision)
        pooled = twin.encode(SENTENCES, batch_size=5, precision=precision)
        assert got.shape == (12, DOUT) and pooled.shape == (12, 64)
        err = H.value_error(got, head_of(pooled, w, b), 64)
        print(f"  encode precision={precision}: share of the value tolerance {err:.3f}")
        assert err <= 1.0
        assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() < 1e-5
    # the same chain from descriptors over the plain checkpoint
    listed = SentenceTransformer(modules=[models.Transformer(tdir), models.Pooling(64),
                                          models.Dense(64, DOUT, init_weight=w, init_bias=b), models.Normalize()], device="cuda")
    assert H.value_error(listed.encode(SENTENCES, batch_size=5), head_of(twin.encode(SENTENCES, batch_size=5), w, b), 64) <= 1.0
    assert np.array_equal(listed.encode(SENTENCES, batch_size=5), model.encode(SENTENCES, batch_size=5))
    # tensors, __call__ and the fused columns go through the same funnel
    t = model.encode(SENTENCES[:3], convert_to_tensor=True)
    assert t.is_cuda and t.shape == (3, DOUT)
    with torch.no_grad():
        out = model(model.tokenize(SENTENCES[:3]))["sentence_embedding"]
    assert out.shape == (3, DOUT)


def test_dimensions(tmp_path):
    ddir, _, _, _ = write_pair(tmp_path)
    model = SentenceTransformer(ddir, device="cuda")
    assert model.get_sentence_embedding_dimension() == DOUT
    assert model.encode([]).shape == (0, DOUT)
    tok = model.encode(SENTENCES[:2], output_value="token_embeddings")
    assert len(tok) == 2 and all(t.shape[1] == 64 for t in tok)          # token embeddings do not pass through the Dense


# ------------------------------------------------------------------ 2. save and reload
def test_save_writes_the_layout_of_sentence_transformers_and_reloads_bit_for_bit(tmp_path):
    ddir, tdir, w, b = write_pair(tmp_path)
    model = SentenceTransformer(ddir, device="cuda")
    out = str(tmp_path / "saved")
    model.save(out)
    mods = json.load(open(os.path.join(out, "modules.json")))
    assert [sorted(m) for m in mods] == [["idx", "name", "path", "type"]] * 4
    assert [m["idx"] for m in mods] == [0, 1, 2, 3] and [m["name"] for m in mods] == ["0", "1", "2", "3"]
    assert [m["path"] for m in mods] == ["", "1_Pooling", "2_Dense", "3_Normalize"] and [m["type"] for m in mods] == TYPES
    assert os.path.isdir(os.path.join(out, "3_Normalize"))
    cfg = json.load(open(os.path.join(out, "2_Dense", "config.json")))
    assert cfg == {"in_features": 64, "out_features": DOUT, "bias": True,
                   "activation_function": "torch.nn.modules.activation.Tanh"}
    sd = torch.load(os.path.join(out, "2_Dense", "pytorch_model.bin"), map_location="cpu", weights_only=True)
    assert sorted(sd) == ["linear.bias", "linear.weight"]
    assert sd["linear.weight"].shape == (DOUT, 64) and sd["linear.bias"].shape == (DOUT,)
    assert torch.equal(sd["linear.weight"], w) and torch.equal(sd["linear.bias"], b)
    again = SentenceTransformer(out, device="cuda")
    assert np.array_equal(again.encode(SENTENCES), model.encode(SENTENCES))
    # a PCA-style head: no bias, no activation, no Normalize behind it
    W = H.dense_tensors(64, 8, bias=False, seed=9)[0]
    pca = SentenceTransformer(modules=[models.Transformer(tdir), models.Pooling(64),
                                       models.Dense(64, 8, bias=False, activation_function=nn.Identity(), init_weight=W)],
                              device="cuda")
    assert [n for n, _ in pca.named_parameters() if n.startswith("2.")] == ["2.linear.weight"]
    twin = SentenceTransformer(tdir, device="cuda")
    assert H.value_error(pca.encode(SENTENCES), head_of(twin.encode(SENTENCES), W, None, H.IDENTITY, 0), 64) <= 1.0
    out2 = str(tmp_path / "saved_pca")
    pca.save(out2)
    mods = json.load(open(os.path.join(out2, "modules.json")))
    assert [m["path"] for m in mods] == ["", "1_Pooling", "2_Dense"] and [m["type"] for m in mods] == TYPES[:3]
    assert json.load(open(os.path.join(out2, "2_Dense", "config.json"))) == {
        "in_features": 64, "out_features": 8, "bias": False, "activation_function": "torch.nn.modules.linear.Identity"}
    sd = torch.load(os.path.join(out2, "2_Dense", "pytorch_model.bin"), map_location="cpu", weights_only=True)
    assert list(sd) == ["linear.weight"] and torch.equal(sd["linear.weight"], W)
    back = SentenceTransformer(out2, device="cuda")
    assert back.get_sentence_embedding_dimension() == 8 and back._dense_normalize is False
    assert np.array_equal(back.encode(SENTENCES), pca.encode(SENTENCES))


# ------------------------------------------------------------------ 3. gradients
def arena_grads(model, feats, upstream):
    """(embedding, the encoder's gradient arena) of one train-mode forward + backward under `upstream` from zeroed buffers.
    upstream: a tensor [B, D], or a function of the embedding that returns one."""
    enc = model._enc
    enc.ensure_train_state()
    enc.grads.zero_()
    if model._dense_params is not None:
        model._dense_params.ensure().zero_grad()
    emb = model({k: v.clone() for k, v in feats.items()})["sentence_embedding"]
    emb.backward(upstream(emb) if callable(upstream) else upstream)
    torch.cuda.synchronize()
    return emb.detach(), enc.grads.clone()


def test_gradients_reach_the_dense_and_the_encoder(tmp_path):
    """Train mode, dropout off, the fp32-class path, loss = (emb * G).sum() with a fixed G. The twin's own run-to-run spread
    is asserted first (at most half the tolerance), so that it is not what the comparison measures."""
    ddir, tdir, w, b = write_pair(tmp_path)
    model, twin = SentenceTransformer(ddir, device="cuda"), SentenceTransformer(tdir, device="cuda")
    for m in (model, twin):
        m.train()
        m.training_precision = "bf16x3"
        assert m._enc.dropout is None
    feats = model.tokenize(SENTENCES)
    G = torch.randn(12, DOUT, generator=torch.Generator().manual_seed(41))
    # the reference head and its gradients, in fp64, on the twin's embedding (of the same train-mode forward)
    pooled, _ = arena_grads(twin, feats, torch.zeros(12, 64, device="cuda"))
    pooled = pooled.cpu()
    assert pooled.shape == (12, 64)
    z, a, ref_y, ref_gx, ref_gw, ref_gb = H.reference_of(pooled, w, b, G, H.TANH, 1)
    assert H.conditions_of(z, a, (ref_gx, ref_gw, ref_gb), H.TANH, 1, DOUT) == []
    up = ref_gx.float().cuda()
    # condition on the test: the twin's backward agrees with itself
    _, first = arena_grads(twin, feats, up)
    _, second = arena_grads(twin, feats, up)
    spread = H.grad_error(second.cpu(), first.cpu())
    print(f"  twin run-to-run spread of the encoder arena: {spread:.3f} of the gradient tolerance")
    assert first.abs().max().item() > 1e-4
    assert spread <= 0.5
    emb, arena = arena_grads(model, feats, G.cuda())
    gw, gb = [p.grad.detach().cpu() for p in dense_params(model)]
    ey = H.value_error(emb, ref_y, 64)
    ew, eb, ea = H.grad_error(gw, ref_gw), H.grad_error(gb, ref_gb), H.grad_error(arena.cpu(), first.cpu())
    print(f"  share of the tolerance: embedding {ey:.3f}, 2.linear.weight.grad {ew:.3f}, 2.linear.bias.grad {eb:.3f}, "
          f"encoder arena against the twin's {ea:.3f}")
    assert ey <= 1.0 and ew <= 1.0 and eb <= 1.0 and ea <= 1.0
    # the .grad of the Dense's parameters are views of the flat buffer the optimiser step reads
    dp = model._dense_params
    assert dense_params(model)[0].grad.data_ptr() == dp.grads.data_ptr() and int(torch.count_nonzero(dp.grads)) > 0
    for m in (model, twin):
        m.training_precision = "bf16"


# ------------------------------------------------------------------ 4. fit
class Recorded(nn.Module):
    """A loss model that keeps the value of every step."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.values = inner, []

    def forward(self, features, labels):
        loss = self.inner(features, labels)
        self.values.append(float(loss.detach()))
        return loss


def teacher_examples(n=16):
    g = torch.Generator().manual_seed(43)
    t = torch.nn.functional.normalize(torch.randn(n, DOUT, generator=g), dim=1)
    return [InputExample(texts=[text(100 + i)], label=t[i].numpy()) for i in range(n)]


def test_fit_trains_the_dense_with_the_encoder(tmp_path):
    ddir, _, w, b = write_pair(tmp_path)
    model = SentenceTransformer(ddir, device="cuda")
    lm = Recorded(S.MSELoss(model))
    p0 = model._enc.params.clone()
    model.fit([(DataLoader(teacher_examples(), batch_size=8), lm)], epochs=10, warmup_steps=0, scheduler="constantlr",
              optimizer_params={"lr": 1e-3}, dropout=0, show_progress_bar=False)
    print(f"  fit MSELoss through Dense: loss {lm.values[0]:.6f} -> {lm.values[-1]:.6f} over {len(lm.values)} steps")
    assert len(lm.values) == 20 and model._enc.opt_step == 20
    assert np.isfinite(lm.values).all() and lm.values[-1] < lm.values[0]
    w1, b1 = [p.detach().cpu() for p in dense_params(model)]
    assert torch.isfinite(w1).all() and torch.isfinite(b1).all() and torch.isfinite(model._enc.params).all()
    assert (w1 - w).abs().max().item() > 1e-4 and (b1 - b).abs().max().item() > 1e-4
    assert not torch.equal(model._enc.params, p0)
    dp = model._dense_params
    assert dense_params(model)[0].data_ptr() == dp.params.data_ptr() and int(torch.count_nonzero(dp.grads)) == 0
    out = str(tmp_path / "fitted")
    model.save(out)
    again = SentenceTransformer(out, device="cuda")
    assert torch.equal(dense_params(again)[0].detach().cpu(), w1)
    assert np.array_equal(again.encode(SENTENCES), model.encode(SENTENCES))


def test_checkpoints_carry_the_dense_and_a_model_without_it_refuses_them(tmp_path):
    ddir, tdir, _, _ = write_pair(tmp_path)
    model, twin = SentenceTransformer(ddir, device="cuda"), SentenceTransformer(tdir, device="cuda")
    ckpt = str(tmp_path / "ckpt")
    model.fit([(DataLoader(teacher_examples(8), batch_size=4), S.MSELoss(model))], epochs=1, warmup_steps=0,
              scheduler="constantlr", optimizer_params={"lr": 1e-3}, dropout=0, show_progress_bar=False, checkpoint_path=ckpt,
              checkpoint_save_steps=2)
    step_dir = os.path.join(ckpt, "2")
    assert [m["path"] for m in json.load(open(os.path.join(step_dir, "modules.json")))] == ["", "1_Pooling", "2_Dense",
                                                                                           "3_Normalize"]
    assert os.path.isfile(os.path.join(step_dir, "2_Dense", "pytorch_model.bin"))
    assert os.path.isfile(os.path.join(step_dir, "training_state.safetensors"))
    assert np.array_equal(SentenceTransformer(step_dir, device="cuda").encode(SENTENCES), model.encode(SENTENCES))
    p0 = twin._enc.params.clone()
    pairs = [InputExample(texts=[text(i), text(60 + i)], label=float(i % 2)) for i in range(8)]
    with pytest.raises(ValueError, match="Dense head"):
        twin.fit([(DataLoader(pairs, batch_size=4), S.CosineSimilarityLoss(twin))], epochs=1, show_progress_bar=False,
                 resume_from_checkpoint=step_dir)
    assert torch.equal(twin._enc.params, p0)


def test_weight_decay_at_a_zero_rate_changes_nothing_and_reaches_the_step(tmp_path):
    ddir, _, _, _ = write_pair(tmp_path)
    model = SentenceTransformer(ddir, device="cuda")
    seen, plain = [], model._enc.adamw_step

    def spy(*args, **kwargs):
        seen.append(kwargs.get("extra"))
        plain(*args, **kwargs)

    model._enc.adamw_step = spy
    p0, x0 = model._enc.params.clone(), model._dense_params.params.clone()
    model.fit([(DataLoader(teacher_examples(8), batch_size=8), S.MSELoss(model))], epochs=1, warmup_steps=0,
              scheduler="constantlr", optimizer_params={"lr": 0.0}, weight_decay=0.1, dropout=0, show_progress_bar=False)
    dp = model._dense_params
    assert seen == [dp] and model._enc.opt_step == 1
    assert torch.equal(model._enc.params, p0) and torch.equal(dp.params, x0)
    # the weight decays, the bias does not: one flag per 256-element chunk of the flat buffer
    flags = dp.chunk_decay.cpu().tolist()
    assert flags == [1] * (64 * DOUT // 256) + [0] and dp.exp_avg is not None


@pytest.mark.parametrize("case", ["SoftmaxLoss", "use_amp", "resume_from_checkpoint"])
def test_what_the_joint_step_cannot_take_is_refused_before_anything_changes(tmp_path, case):
    ddir, _, _, _ = write_pair(tmp_path)
    model = SentenceTransformer(ddir, device="cuda")
    kwargs, lm, data = {}, S.MSELoss(model), teacher_examples(8)
    if case == "SoftmaxLoss":
        lm = S.SoftmaxLoss(model, model.get_sentence_embedding_dimension(), 2)
        data = [InputExample(texts=[text(i), text(50 + i)], label=i % 2) for i in range(8)]
    elif case == "use_amp":
        kwargs = {"use_amp": True}
    else:
        kwargs = {"resume_from_checkpoint": str(tmp_path / "no_such_checkpoint")}
    p0, x0, step0 = model._enc.params.clone(), model._dense_params.params.clone(), model._enc.opt_step
    with pytest.raises(NotImplementedError, match=f"Dense.*{case}"):
        model.fit([(DataLoader(data, batch_size=4), lm)], epochs=1, warmup_steps=0, scheduler="constantlr", dropout=0,
                  show_progress_bar=False, **kwargs)
    assert torch.equal(model._enc.params, p0) and torch.equal(model._dense_params.params, x0)
    assert model._enc.opt_step == step0 and model.training_precision == "bf16" and model._dp is None
