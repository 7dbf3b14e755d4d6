"""GPU: the RoBERTa encoder architecture (QST_ARCH_ROBERTA), the classification-head kernel (qst_cls_head_fwd) and
CrossEncoder.predict end to end, each against fp32 / fp64 torch and the installed transformers."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quadruplet_sentence_transformer_amd  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib  # noqa: E402
from quadruplet_sentence_transformer_amd.config import PRESETS, build_layout, hf_param_views  # noqa: E402
from quadruplet_sentence_transformer_amd.encoder import HipEncoder  # noqa: E402
from cross_encoder_fixtures import CORPUS, ROBERTA_VOCAB, make_checkpoint  # noqa: E402


# ---------------------------------------------------------------------------------------------------- head kernel
def head_ref(x, w1, b1, w2, b2, act, softmax):
    x, w1, b1, w2, b2 = (t.double() for t in (x, w1, b1, w2, b2))
    z = torch.tanh(x @ w1.t() + b1) @ w2.t() + b2
    if act == 1:
        z = torch.sigmoid(z)
    if softmax and z.shape[1] > 1:
        z = torch.softmax(z, dim=1)
    return z


def run_head(x, w1, b1, w2, b2, act, softmax, ldx=None):
    lib = _lib.load()
    n, C = x.shape[0], w2.shape[0]
    out = torch.full((n, C), float("nan"), device="cuda")
    st = lib.qst_cls_head_fwd(x.data_ptr(), ldx or x.shape[1], n, w1.shape[0], w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                              b2.data_ptr(), C, act, softmax, out.data_ptr(), _lib.current_stream_ptr())
    return st, out


@pytest.mark.parametrize("H", [64, 384, 768, 1024])
@pytest.mark.parametrize("n", [1, 33, 1000])
def test_head_kernel_matches_fp64(H, n):
    g = torch.Generator().manual_seed(H + n)
    # x with a row stride wider than H (the encoder's out_emb may be a slice of a wider buffer)
    xw = torch.randn(n, H + 64, generator=g)
    w1, b1 = torch.randn(H, H, generator=g) / H ** 0.5, 0.1 * torch.randn(H, generator=g)
    for C in (1, 3):
        w2, b2 = torch.randn(C, H, generator=g) / H ** 0.5, 0.1 * torch.randn(C, generator=g)
        dev = [t.cuda().contiguous() for t in (xw, w1, b1, w2, b2)]
        for act in (0, 1):
            for softmax in (0, 1):
                st, out = run_head(*dev, act, softmax, ldx=H + 64)
                torch.cuda.synchronize()
                assert st == 0
                ref = head_ref(xw[:, :H], w1, b1, w2, b2, act, softmax)
                torch.testing.assert_close(out.cpu().double(), ref, rtol=1e-5, atol=2e-6)


def test_head_kernel_refuses_bad_arguments():
    lib = _lib.load()
    H, C, n = 64, 3, 4
    x, w1, b1 = torch.randn(n, H, device="cuda"), torch.randn(H, H, device="cuda"), torch.randn(H, device="cuda")
    w2, b2, out = torch.randn(9, H, device="cuda"), torch.randn(9, device="cuda"), torch.zeros(n, 9, device="cuda")
    s = _lib.current_stream_ptr()
    call = lambda **k: lib.qst_cls_head_fwd(k.get("x", x.data_ptr()), k.get("ldx", H), k.get("n", n), k.get("H", H),  # noqa: E731
                                            k.get("w1", w1.data_ptr()), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                            k.get("C", C), k.get("act", 0), k.get("softmax", 0), out.data_ptr(), s)
    assert call() == 0
    assert call(C=9) == -1 and call(C=0) == -1 and call(act=2) == -1 and call(softmax=3) == -1
    assert call(x=None) == -1 and call(w1=None) == -1 and call(n=0) == -1 and call(ldx=H - 1) == -1
    assert call(w1=w1.data_ptr() + 4) == -1                       # W1 is read as float4 runs
    big = torch.zeros(1088 * 1088, device="cuda")
    assert call(H=1088, ldx=1088, w1=big.data_ptr()) == -2 and call(H=66, ldx=66) == -2
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- RoBERTa encoder
def hf_roberta(cfg, seed, std):
    import transformers as T
    hc = T.RobertaConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_layers,
                         num_attention_heads=cfg.num_heads, intermediate_size=cfg.intermediate_size,
                         max_position_embeddings=cfg.max_position, type_vocab_size=cfg.type_vocab_size, pad_token_id=1,
                         layer_norm_eps=cfg.layer_norm_eps, hidden_act="gelu")
    m = T.RobertaModel(hc, add_pooling_layer=False).eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("LayerNorm.weight"):
                p.copy_(1.0 + 0.05 * torch.randn(p.shape, generator=g))
            elif name.endswith("bias"):
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(std * torch.randn(p.shape, generator=g))
    return m


def arena_from(model, cfg):
    sd = model.state_dict()
    segs, total = build_layout(cfg)
    so = {s.name: s for s in segs}
    arena = np.zeros(total, np.float32)
    for name, seg, off, shape in hf_param_views(cfg):
        s = so[seg]
        arena[s.offset + off:s.offset + off + int(np.prod(shape))] = sd[name].numpy().reshape(-1)
    return arena


def ragged_ids(cfg, lens, L, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(lens), L), cfg.pad_token_id, dtype=torch.int64)
    mask = torch.zeros(len(lens), L, dtype=torch.int64)
    for i, n in enumerate(lens):
        ids[i, :n] = torch.randint(3, cfg.vocab_size, (n,), generator=g)
        ids[i, 0], ids[i, n - 1] = 0, 2                                   # <s> ... </s>
        mask[i, :n] = 1
    return ids, mask


@pytest.mark.parametrize("name,std,lens,L", [("tiny-roberta", 0.08, [64, 37, 5, 20], 64),
                                             ("roberta-large-2l", 0.02, [64, 41, 7], 64)])
def test_roberta_encoder_matches_hf(name, std, lens, L):
    from dataclasses import replace
    cfg = replace(PRESETS[name], pooling="cls")
    model = hf_roberta(cfg, seed=5, std=std)
    ids, mask = ragged_ids(cfg, lens, L, seed=5)
    with torch.no_grad():
        ref_tok = model(input_ids=ids, attention_mask=mask).last_hidden_state
    enc = HipEncoder(cfg)
    enc.load_arena(arena_from(model, cfg))
    idd, mdd = ids.cuda(), mask.cuda()
    m3 = mask.bool().unsqueeze(-1)
    sc = float(ref_tok[:, 0].norm(dim=-1).mean())          # no Normalize module: tolerances on the embedding's scale
    for prec in ("bf16x3", "bf16", "f16", "f16w", "fp8"):
        if prec == "fp8" and cfg.hidden_size % 128:
            continue                                         # fp8 takes 128-deep K stages (qst_encoder_create)
        emb, tok, _ = enc.forward(idd, mdd, None, training=False, want_tokens=True, precision=prec)
        torch.cuda.synchronize()
        emb, tok = emb.cpu(), tok.cpu()
        if prec == "bf16x3":
            torch.testing.assert_close(emb, ref_tok[:, 0], rtol=1e-3, atol=1e-4)
            torch.testing.assert_close(tok * m3, ref_tok * m3, rtol=1e-3, atol=1e-4)
        else:
            bound = (2e-3 if prec in ("bf16", "f16", "f16w") else 2e-2) * sc
            assert (emb - ref_tok[:, 0]).abs().max().item() < bound, prec


# ---------------------------------------------------------------------------------------------------- CrossEncoder
def hf_scores(model, tok, pairs, act, softmax=False):
    a, b = [p[0].strip() for p in pairs], [p[1].strip() for p in pairs]
    f = tok(a, b, padding=True, truncation="longest_first", return_tensors="pt", max_length=64)
    with torch.no_grad():
        z = act(model(**f).logits.double())
    if softmax and z.shape[1] > 1:
        z = torch.softmax(z, dim=1)
    return z


@pytest.mark.parametrize("kind", ["bert", "roberta", "xlm-roberta"])
def test_cross_encoder_predict_matches_hf(tmp_path, kind):
    from transformers import AutoTokenizer
    from quadruplet_sentence_transformer_amd.cross_encoder import CrossEncoder
    d = str(tmp_path / kind)
    model = make_checkpoint(d, kind, num_labels=1, seed=3)
    tok = AutoTokenizer.from_pretrained(d, local_files_only=True)
    # unsorted lengths, a duplicate, surrounding white space: the result must come back in input order
    pairs = [(CORPUS[i % 10], CORPUS[(3 * i + 1) % 10] + " " * (i % 2)) for i in range(23)]
    pairs[5] = ("  " + pairs[5][0], "short")
    ce = CrossEncoder(d, precision="bf16x3")
    got = ce.predict(pairs, batch_size=8)
    ref = hf_scores(model, tok, pairs, torch.sigmoid)[:, 0]
    assert isinstance(got, np.ndarray) and got.shape == (23,)
    np.testing.assert_allclose(got, ref.numpy(), rtol=1e-3, atol=1e-4)
    # bf16 (the default): same order, looser values
    got16 = CrossEncoder(d).predict(pairs, batch_size=5)
    assert np.abs(got16 - ref.numpy()).max() < 2e-2
    # a single pair -> a scalar; convert_to_tensor; Identity; a custom callable on the raw logits
    one = ce.predict(list(pairs[3]))
    assert np.ndim(one) == 0 and abs(float(one) - float(ref[3])) < 1e-4 + 1e-3 * abs(float(ref[3]))
    t = ce.predict(pairs, convert_to_tensor=True, activation_fct=torch.nn.Identity())
    assert torch.is_tensor(t) and t.shape == (23,)
    logits = hf_scores(model, tok, pairs, lambda z: z)[:, 0]
    np.testing.assert_allclose(t.cpu().numpy(), logits.numpy(), rtol=1e-3, atol=1e-4)
    tanh = ce.predict(pairs, activation_fct=torch.tanh)
    np.testing.assert_allclose(tanh, np.tanh(logits.numpy()), rtol=1e-3, atol=1e-4)


def test_cross_encoder_three_labels_with_softmax(tmp_path):
    from transformers import AutoTokenizer
    from quadruplet_sentence_transformer_amd.cross_encoder import CrossEncoder
    d = str(tmp_path / "nli")
    model = make_checkpoint(d, "roberta", num_labels=3, seed=9)
    tok = AutoTokenizer.from_pretrained(d, local_files_only=True)
    pairs = [(CORPUS[i], CORPUS[(i + 4) % 10]) for i in range(10)]
    ce = CrossEncoder(d, precision="bf16x3")
    assert isinstance(ce.default_activation_function, torch.nn.Identity)
    got = ce.predict(pairs, apply_softmax=True, batch_size=4)
    assert got.shape == (10, 3)
    np.testing.assert_allclose(got, hf_scores(model, tok, pairs, lambda z: z, softmax=True).numpy(), rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(got.sum(1), np.ones(10), atol=1e-5)
    row = ce.predict(list(pairs[2]), apply_softmax=True, convert_to_tensor=True)
    assert torch.is_tensor(row) and row.shape == (3,)
    np.testing.assert_allclose(row.cpu().numpy(), got[2], rtol=0, atol=1e-6)


def test_reference_ir_call_shape_through_the_dropin(tmp_path):
    """models/evaluators.py:501-508: predict over a list of [query, doc] lists, then scores >= threshold pick the relevant
    documents -- through the drop-in sentence_transformers namespace, with no placeholder error."""
    from transformers import AutoTokenizer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = str(tmp_path / "stsb")
    model = make_checkpoint(d, "roberta", num_labels=1, seed=4)
    tok = AutoTokenizer.from_pretrained(d, local_files_only=True)
    sys.path.insert(0, os.path.join(root, "dropin"))
    try:
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]
        from sentence_transformers import CrossEncoder
        from sentence_transformers.cross_encoder import CrossEncoder as CE2
        assert CE2 is CrossEncoder
        ce = CrossEncoder(d, precision="bf16x3")
        queries, corpus = CORPUS[:3], CORPUS
        for q in queries:
            pairs = [[q, c] for c in corpus]
            scores = ce.predict(pairs)
            ref = hf_scores(model, tok, pairs, torch.sigmoid)[:, 0].numpy()
            thr = float(np.median(ref))
            far = np.abs(ref - thr) > 1e-3                     # pairs whose side of the threshold rounding cannot flip
            np.testing.assert_array_equal((scores >= thr)[far], (ref >= thr)[far])
    finally:
        sys.path.remove(os.path.join(root, "dropin"))
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]


# ---------------------------------------------------------------------------------------------------- RoBERTa bi-encoder
def test_roberta_sentence_transformer_encode_and_backward_match_hf(tmp_path):
    import transformers as T
    from cross_encoder_fixtures import bpe_tokenizer_files
    from quadruplet_sentence_transformer_amd.sentence_transformer import SentenceTransformer
    from dataclasses import replace
    cfg = replace(PRESETS["tiny-roberta"], vocab_size=ROBERTA_VOCAB)        # the byte-level BPE's 290 ids
    model = hf_roberta(cfg, seed=11, std=0.08)
    d = str(tmp_path / "bi")
    os.makedirs(d)
    model.save_pretrained(d, safe_serialization=True)
    bpe_tokenizer_files(d)
    tok = T.AutoTokenizer.from_pretrained(d, local_files_only=True)
    st = SentenceTransformer(d, device="cuda")
    assert st.cfg.arch == 2 and st.cfg.type_vocab_size == 1 and st.cfg.layer_norm_eps == 1e-5
    texts = CORPUS[:7]
    f = tok(texts, padding=True, truncation="longest_first", return_tensors="pt", max_length=64)

    def hf_mean(m):
        h = m(input_ids=f["input_ids"], attention_mask=f["attention_mask"]).last_hidden_state
        w = f["attention_mask"].unsqueeze(-1).float()
        return (h * w).sum(1) / w.sum(1)
    with torch.no_grad():
        ref = hf_mean(model)
    got = st.encode(texts, precision="bf16x3", convert_to_tensor=True).cpu()
    torch.testing.assert_close(got, ref, rtol=1e-3, atol=1e-4)
    # one bf16x3 training backward against HF autograd
    g = torch.Generator().manual_seed(2)
    w = torch.randn(len(texts), cfg.hidden_size, generator=g)
    ref_loss = (hf_mean(model) * w).sum()
    ref_loss.backward()
    st.train()
    st.training_precision = "bf16x3"
    st._enc.grads.zero_()
    feats = st.tokenize(texts)
    emb = st(feats)["sentence_embedding"]
    (emb * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    params = dict(st.named_parameters())
    gnorm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.parameters())))
    for name, p in model.named_parameters():
        got_g = params["0.auto_model." + name].grad.cpu()
        ref_g = p.grad
        if name == "embeddings.position_embeddings.weight":
            ref_g, got_g = ref_g[cfg.pad_token_id + 1:], got_g[cfg.pad_token_id + 1:]     # the rows real tokens use
            assert ref_g.norm() > 0
        denom = ref_g.norm().item()
        if denom <= 1e-5 * gnorm:
            assert got_g.norm().item() <= 1e-5 * gnorm, name
            continue
        err = ((got_g - ref_g).norm() / max(denom, 1e-3 * gnorm)).item()
        assert err < 1e-4, f"{name}: relative L2 error {err:.3e}"
    # save() writes model_type roberta: the directory loads back as the same model
    out = str(tmp_path / "saved")
    st.save(out)
    st2 = SentenceTransformer(out, device="cuda")
    assert st2.cfg.arch == 2
    torch.testing.assert_close(st2.encode(texts, precision="bf16x3", convert_to_tensor=True).cpu(), got, rtol=0, atol=1e-6)
