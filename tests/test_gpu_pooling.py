"""GPU: the pooling heads of sentence-transformers 2.2.2 (cls, max, mean, mean_sqrt_len, weightedmean, concatenated in
that order) -- qst_pool_fwd/bwd against a torch restatement of models.Pooling.forward and, bit for bit, against digests
recorded before the mean head's own kernel pair was folded into them, the encoder against the HF token states, training
through every path, and the public surface."""
import json
import os
from dataclasses import replace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import quadruplet_sentence_transformer_amd  # noqa: F401
from quadruplet_sentence_transformer_amd import _lib, models
from quadruplet_sentence_transformer_amd.config import POOLING_MODES, PRESETS, build_layout, pooling_mask, pooling_modes
from quadruplet_sentence_transformer_amd.encoder import HipEncoder
from quadruplet_sentence_transformer_amd.synthetic import synthetic_params, synthetic_quadruplets
from quadruplet_sentence_transformer_amd.trainer import QuadrupletTrainer, warmup_linear_lr
from oracle import torch_ref as R
from kernel_helpers import lib, quad_batch  # noqa: F401
import pool_digest_cases as P

pytestmark = pytest.mark.gpu

LOSS_KW = dict(gamma=0.6, margin_pos_neg=1.0, margin_pos_part=0.5, margin_part_neg=0.5, p=2.0, swap=False)
HEADS = ["cls", "max", "mean", "mean_sqrt_len", "weightedmean", "cls+mean", "max+mean+mean_sqrt_len", "+".join(POOLING_MODES)]


def st_pool(tok, mask, pooling, normalize):
    """sentence-transformers 2.2.2 models.Pooling.forward (+ Normalize), restated: tok [n, L, H] fp32, mask [n, L]."""
    m = mask[:, :, None].to(tok.dtype)
    L = tok.shape[1]
    out = []
    for mode in pooling_modes(pooling):
        if mode == "cls":
            out.append(tok[:, 0])
        elif mode == "max":
            out.append(tok.masked_fill(m == 0, -1e9).max(1).values)      # ST fills padding with -1e9 in place, then max
        elif mode == "mean":
            out.append((tok * m).sum(1) / m.sum(1).clamp(min=1e-9))
        elif mode == "mean_sqrt_len":
            out.append((tok * m).sum(1) / torch.sqrt(m.sum(1).clamp(min=1e-9)))
        else:
            w = torch.arange(1, L + 1, dtype=tok.dtype, device=tok.device)[None, :, None] * m
            out.append((tok * w).sum(1) / w.sum(1).clamp(min=1e-9))
    e = torch.cat(out, 1)
    return F.normalize(e, p=2, dim=1, eps=1e-12) if normalize else e


def ragged_mask(n, L, gen):
    """Row 0 all padding, row 1 full, the rest of random lengths (right-padded)."""
    lens = torch.randint(1, L + 1, (n,), generator=gen)
    lens[0], lens[1] = 0, L
    return (torch.arange(L)[None, :] < lens[:, None]).to(torch.int64)


def pool_fwd(lib, tok, mask, mode, normalize, H):
    n, L, _ = tok.shape
    D = bin(mode).count("1") * H
    emb = torch.full((n, D), float("nan"), device="cuda")
    pooled = torch.full((n, D), float("nan"), device="cuda")
    argmax = torch.full((n, H), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.qst_pool_fwd(tok.data_ptr(), mask.data_ptr(), n, L, H, mode, int(normalize), emb.data_ptr(), pooled.data_ptr(),
                                argmax.data_ptr(), _lib.current_stream_ptr()), "qst_pool_fwd")
    return emb, pooled, argmax


def pool_bwd(lib, demb, pooled, argmax, mask, mode, normalize, L, H):
    n = demb.shape[0]
    dtok = torch.full((n, L, H), float("nan"), device="cuda")
    _lib.check(lib.qst_pool_bwd(demb.data_ptr(), pooled.data_ptr(), argmax.data_ptr(), mask.data_ptr(), n, L, H, mode, int(normalize),
                                dtok.data_ptr(), _lib.current_stream_ptr()), "qst_pool_bwd")
    return dtok


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("pooling", HEADS)
def test_pool_kernels_match_torch(lib, pooling, normalize):
    mode = pooling_mask(pooling)
    gen = torch.Generator().manual_seed(5 + mode)
    for H in (64, 384, 768, 1024):
        for L in (32, 128, 512):
            n = 6
            tok = torch.randn(n, L, H, generator=gen).cuda()               # continuous random: no ties
            mask = ragged_mask(n, L, gen).cuda()
            t = tok.clone().requires_grad_(True)
            ref = st_pool(t, mask, pooling, normalize)
            demb = torch.randn(ref.shape, generator=gen).cuda()
            ref.backward(demb)
            emb, pooled, argmax = pool_fwd(lib, tok, mask, mode, normalize, H)
            torch.testing.assert_close(emb, ref.detach(), rtol=1e-5, atol=1e-6, msg=f"fwd H={H} L={L}")
            torch.testing.assert_close(pooled, st_pool(tok, mask, pooling, False), rtol=1e-5, atol=1e-6)
            if mode & 2:
                m = mask.bool()[:, :, None]
                ref_idx = tok.masked_fill(~m, -1e9).max(1).indices.to(torch.int32)
                ref_idx[mask.sum(1) == 0] = -1
                assert torch.equal(argmax, ref_idx)
            dtok = pool_bwd(lib, demb, pooled, argmax, mask, mode, normalize, L, H)
            torch.testing.assert_close(dtok, t.grad, rtol=1e-5, atol=1e-6, msg=f"bwd H={H} L={L}")


def test_max_ties_go_to_the_lowest_token_index(lib):
    """Tied maxima, in rows owned by one wave (1, 9) and by different waves (2, 5, 13 / 7, 3): the argmax is the lowest
    valid row and the column's whole gradient lands there."""
    n, L, H = 2, 32, 64
    tok = -torch.rand(n, L, H).cuda()                                      # everything below the ties
    mask = torch.ones(n, L, dtype=torch.int64).cuda()
    mask[1, 3] = 0                                                          # (a tie on a padding row does not count)
    for r in (2, 5, 13):
        tok[:, r, 0] = 2.0
    for r in (9, 1):
        tok[:, r, 1] = 3.0
    for r in (7, 3):
        tok[:, r, 2] = 1.5
    emb, pooled, argmax = pool_fwd(lib, tok, mask, 2, False, H)
    assert argmax[:, :3].tolist() == [[2, 1, 3], [2, 1, 7]]
    demb = torch.randn(n, H).cuda()
    dtok = pool_bwd(lib, demb, pooled, argmax, mask, 2, False, L, H)
    for s in range(n):
        for c, r in zip(range(3), argmax[s, :3].tolist()):
            col = dtok[s, :, c]
            assert col[r] == demb[s, c] and int((col != 0).sum()) == 1


def test_every_head_reproduces_the_digests_of_the_two_pair_kernels(lib, golden_dir):
    """Bitwise, on every head: each case of tests/pool_digest_cases.py run on the tree's library gives the SHA-256 of emb,
    pooled, argmax and dtok that tests/golden/pool_digests.json recorded (tools/pool_digest.py) on the library of the commit
    named there, whose mean head still ran its own kernel pair."""
    want = json.load(open(os.path.join(golden_dir, "pool_digests.json")))["cases"]
    assert sorted(want) == sorted(P.case_name(*c) for c in P.CASES), "the recorded cases are not the cases of pool_digest_cases.py"
    different = []
    for case in P.CASES:
        name = P.case_name(*case)
        got = P.run_case(lib.qst_pool_fwd, lib.qst_pool_bwd, *case, stream=_lib.current_stream_ptr())
        assert got["inputs"] == want[name]["inputs"], f"{name}: inputs changed, not the kernel"
        different += [f"{name}: {k}" for k in want[name] if got.get(k) != want[name][k]]
        assert set(got) == set(want[name]), name
    assert not different, different


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_default_encoder_still_runs_the_old_mean_kernel(lib, precision):
    """An encoder left at the default head: its embeddings are BITWISE those of qst_pool_fwd(mode = QST_POOL_MEAN) on its own
    token states."""
    cfg = PRESETS["tiny-bert"]
    enc = HipEncoder(cfg, device="cuda:0")
    enc.load_arena(synthetic_params(cfg, seed=14, std=0.05))
    ids, mask, types = [torch.from_numpy(x).cuda().view(-1, 64) for x in synthetic_quadruplets(cfg, 3, 64, seed=14, ragged=True)]
    emb, tok, _ = enc.forward(ids, mask, types, want_tokens=True, precision=precision)
    n, L, H = tok.shape
    ref, _, _ = pool_fwd(lib, tok, mask, pooling_mask("mean"), True, H)
    assert torch.equal(emb, ref)
    assert lib.qst_encoder_embedding_dim(enc.handle) == H


def golden_cases():
    return [("tinybert_hfinit", "tiny-bert", 2, 32, dict(std=0.02)),
            ("tinybert_trained", "tiny-bert", 3, 64, dict(std=0.08, bias_std=0.05, ln_jitter=0.1)),
            ("tinympnet_trained", "tiny-mpnet", 2, 64, dict(std=0.08, bias_std=0.05, ln_jitter=0.1)),
            ("tinybert_maskedge", "tiny-bert", 3, 64, dict(std=0.08, bias_std=0.05, ln_jitter=0.1)),
            ("tinympnet_maskedge", "tiny-mpnet", 3, 64, dict(std=0.08, bias_std=0.05, ln_jitter=0.1))]


@pytest.mark.parametrize("pooling", HEADS)
def test_encoder_heads_match_st_on_the_hf_token_states(golden_dir, pooling):
    from tests.test_oracle_golden import golden_inputs
    g = np.load(os.path.join(golden_dir, "encoder_golden.npz"))
    for key, preset, B, L, wkw in golden_cases():
        cfg = replace(PRESETS[preset], pooling=pooling)
        enc = HipEncoder(cfg, device="cuda:0")
        enc.load_arena(synthetic_params(cfg, seed=14, **wkw))
        ids, mask, types = golden_inputs(key, cfg, B, L)
        n = 4 * B
        mask_t = torch.from_numpy(mask).view(n, L)
        emb, tok, _ = enc.forward(*quad_batch(cfg, ids, mask, types, B, L), want_tokens=True, precision="bf16x3")
        assert emb.shape == (n, cfg.embedding_dim)
        hf_tok = torch.from_numpy(g[key + "_tok"]).view(n, L, cfg.hidden_size)
        ref = st_pool(hf_tok, mask_t, pooling, cfg.normalize)
        got = emb.cpu()
        valid = mask_t.sum(1) > 0
        torch.testing.assert_close(got[valid], ref[valid], rtol=1e-3, atol=1e-4, msg=key)
        if (~valid).any():
            assert torch.isfinite(got[~valid]).all()
            H = cfg.hidden_size
            o = 0
            for mode in pooling_modes(pooling):                 # all-padding rows: exactly what ST gives, cls only finite
                if mode != "cls":
                    blk = st_pool(hf_tok[~valid], mask_t[~valid], pooling, cfg.normalize)[:, o * H:(o + 1) * H]
                    torch.testing.assert_close(got[~valid][:, o * H:(o + 1) * H], blk, rtol=1e-3, atol=1e-4)
                o += 1


def oracle_step(P, cfg, t, masks=None):
    four, B, L = t[0].shape
    ids, mask, types = (x.reshape(4 * B, L) for x in t)
    tok = R.encoder_forward(P, cfg, ids, mask, types, False, dropout=masks)
    emb = st_pool(tok, mask, cfg.pooling, cfg.normalize).view(4, B, -1)
    return R.gamma_quadruplet_loss_ref(emb[0], emb[1], emb[2], emb[3], **LOSS_KW)


@pytest.mark.parametrize("pooling", ["cls", "max+mean"])
def test_parity_training_with_other_heads_tracks_the_fp32_reference(pooling):
    cfg = replace(PRESETS["tiny-bert"], pooling=pooling)
    B, L, steps, lr, warmup, total = 6, 32, 6, 2e-3, 2, 20
    arena = synthetic_params(cfg, seed=14, std=0.05, bias_std=0.02, ln_jitter=0.05)
    P = R.arena_to_dict(arena, cfg, requires_grad=True)
    segs, _ = build_layout(cfg)
    groups = [{"params": [P[s.name] for s in segs if s.decay], "weight_decay": 0.01},
              {"params": [P[s.name] for s in segs if not s.decay], "weight_decay": 0.0}]
    opt = torch.optim.AdamW(groups, lr=lr, betas=(0.9, 0.999), eps=1e-8)
    tr = QuadrupletTrainer(cfg, arena=arena, device="cuda:0", lr=lr, weight_decay=0.01, max_grad_norm=1.0,
                           warmup_steps=warmup, total_steps=total, precision="bf16x3", **LOSS_KW)
    ref_losses, hip_losses = [], []
    for step in range(steps):
        t = [torch.from_numpy(x) for x in synthetic_quadruplets(cfg, B, L, seed=14, ragged=True, step=0)]
        for g in opt.param_groups:
            g["lr"] = warmup_linear_lr(lr, step, warmup, total)
        opt.zero_grad()
        loss = oracle_step(P, cfg, t)
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p for g in opt.param_groups for p in g["params"]], 1.0)
        opt.step()
        ref_losses.append(loss.item())
        hip_losses.append(tr.step(*[x.cuda() for x in t]).item())
    assert ref_losses[-1] < ref_losses[0] - 0.01, "reference did not train"
    np.testing.assert_allclose(hip_losses, ref_losses, rtol=0, atol=1e-4)


@pytest.mark.parametrize("precision", ["bf16", "f16", "f16w", "fp8"])
@pytest.mark.parametrize("pooling", ["cls", "max"])
def test_reduced_precisions_train_with_other_heads(precision, pooling):
    cfg = replace(PRESETS["all-MiniLM-L6-v2"], num_layers=2, vocab_size=2048, pooling=pooling)
    arena = synthetic_params(cfg, seed=14, std=0.05, bias_std=0.02, ln_jitter=0.05)
    tr = QuadrupletTrainer(cfg, arena=arena, device="cuda:0", lr=2e-3, precision=precision, **LOSS_KW)
    t = [torch.from_numpy(x).cuda() for x in synthetic_quadruplets(cfg, 8, 32, seed=14, ragged=True)]
    losses = [tr.step(*t).item() for _ in range(6)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert torch.isfinite(tr.enc.params).all()


@pytest.mark.parametrize("pooling", ["cls", "max+mean"])
def test_graph_replayed_steps_match_eager_steps_with_other_heads(pooling):
    cfg = replace(PRESETS["tiny-bert"], pooling=pooling)
    lr, warmup, total = 2e-3, 3, 12
    arena = synthetic_params(cfg, seed=14, std=0.05, bias_std=0.02, ln_jitter=0.05)
    kw = dict(arena=arena, device="cuda:0", lr=lr, weight_decay=0.01, max_grad_norm=1.0, warmup_steps=warmup,
              total_steps=total, **LOSS_KW)
    eager, graph = QuadrupletTrainer(cfg, **kw), QuadrupletTrainer(cfg, use_graph=True, **kw)
    le, lg = [], []
    for step in range(8):
        t = [torch.from_numpy(x).cuda() for x in synthetic_quadruplets(cfg, 6, 32, seed=14, ragged=True, step=step % 4)]
        le.append(eager.step(*t).item())
        lg.append(graph.step(*t).item())
    assert len(graph._graphs) == 1
    assert abs(lg[0] - le[0]) < 1e-6
    np.testing.assert_allclose(lg, le, rtol=0, atol=2e-3)


@pytest.mark.parametrize("pooling", ["cls", "max+mean", "+".join(POOLING_MODES)])
def test_staged_backward_over_rccl_matches_one_call(pooling):
    """World size 1 over the library's own RCCL communicator: the data-parallel staged backward (per-layer stages, layer 0's
    postponed weight gradients, one all-reduce per bucket) gives the gradients of the one-call backward."""
    from quadruplet_sentence_transformer_amd.comm import NativeComm
    from quadruplet_sentence_transformer_amd.encoder import stacked
    from quadruplet_sentence_transformer_amd.trainer import gradient_buckets, staged_backward
    torch.cuda.set_device(0)
    cfg = replace(PRESETS["all-MiniLM-L6-v2"], num_layers=2, vocab_size=4096, pooling=pooling)
    arena = synthetic_params(cfg, seed=14, std=0.05, bias_std=0.02, ln_jitter=0.05)
    batch = [torch.from_numpy(x).cuda() for x in synthetic_quadruplets(cfg, 32, 128, seed=14, ragged=True)]
    comm = NativeComm(0, 1, NativeComm.unique_id())
    out = []
    for mode in ("oneshot", "staged"):
        tr = QuadrupletTrainer(cfg, arena=arena, device="cuda:0")
        enc = tr.enc
        enc.grads.zero_()
        loss, _, g, saved, (ids, mask, types) = tr.forward_loss(*batch, training=True, want_grads=True)
        if mode == "oneshot":
            enc.backward(ids, mask, types, stacked(g), saved)
        else:
            for w in staged_backward(enc, ids, mask, types, stacked(g), saved, None, gradient_buckets(cfg), comm, True):
                w.wait()
        torch.cuda.synchronize()
        out.append(enc.grads.cpu().numpy())
    g1, g2 = out
    assert np.isfinite(g1).all() and np.isfinite(g2).all()
    gnorm = float(np.linalg.norm(g1))
    for s in build_layout(cfg)[0]:
        a, b = g1[s.offset:s.offset + s.numel], g2[s.offset:s.offset + s.numel]
        na = float(np.linalg.norm(a))
        if na <= 1e-6 * gnorm:
            assert float(np.linalg.norm(b)) <= 1e-5 * gnorm, s.name
            continue
        assert float(np.linalg.norm(a - b)) <= 1e-5 * na + 1e-9, s.name


def test_backward_refuses_an_arena_of_another_head():
    cfg = replace(PRESETS["tiny-bert"], pooling="cls+max")
    enc = HipEncoder(cfg, device="cuda:0")
    enc.load_arena(synthetic_params(cfg, seed=1))
    ids, mask, types = [torch.from_numpy(x).cuda().view(-1, 32) for x in synthetic_quadruplets(cfg, 2, 32, seed=1, ragged=True)]
    emb, _, saved = enc.forward(ids, mask, types, training=True)
    assert emb.shape == (8, 128)
    lib = enc.lib
    _lib.check(lib.qst_encoder_set_pooling(enc.handle, pooling_mask("cls")))
    with pytest.raises(_lib.QstError, match="bad argument"):
        enc.backward(ids, mask, types, torch.ones(8, 64, device="cuda"), saved)
    _lib.check(lib.qst_encoder_set_pooling(enc.handle, pooling_mask("cls+max")))
    enc.backward(ids, mask, types, torch.ones_like(emb), saved)
    torch.cuda.synchronize()
    assert torch.isfinite(enc.grads).all()


def test_sentence_transformer_with_a_cls_head_encodes_fits_saves_and_reloads(tmp_path):
    from quadruplet_sentence_transformer_amd.losses import GammaQuadrupletLoss
    from quadruplet_sentence_transformer_amd.quadruplet_model import QuadrupletSentenceTransformerLossModel
    from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample, SentenceTransformer
    from tests.test_pooling_host import write_tiny_bert
    src = str(tmp_path / "plain")
    write_tiny_bert(src, st_files=False)
    model = SentenceTransformer(modules=[models.Transformer(src, max_seq_length=48), models.Pooling(64, pooling_mode="cls"),
                                         models.Normalize()], device="cuda:0")
    assert model.cfg.pooling == "cls" and model.cfg.normalize and model.get_sentence_embedding_dimension() == 64
    texts = [f"sentence number {i} " + "word " * (i % 7) for i in range(10)]
    e0 = model.encode(texts, batch_size=4)
    assert e0.shape == (10, 64) and np.allclose(np.linalg.norm(e0, axis=1), 1.0, atol=1e-5)
    toks = model.encode(texts[:3], output_value="token_embeddings", convert_to_numpy=False)
    feats = model.tokenize(texts[:3])
    ids, mask = feats["input_ids"].cuda(), feats["attention_mask"].cuda()
    ids_p, mask_p, types_p, _ = HipEncoder.pad_inputs(ids, mask, feats["token_type_ids"].cuda(), 0)
    _, tok, _ = model._enc.forward(ids_p, mask_p, types_p, want_tokens=True)
    for i, t in enumerate(toks):
        n = int(mask[i].sum())
        assert t.shape == (n, 64) and torch.equal(t, tok[i, :n])
    # fit (the quadruplet loss on the cls head), then save and reload
    data = [InputExample(texts=[texts[i], texts[(i + 1) % 10], texts[(i + 2) % 10], texts[(i + 5) % 10]]) for i in range(8)]
    loader = torch.utils.data.DataLoader(data, batch_size=4, shuffle=False)
    lm = QuadrupletSentenceTransformerLossModel(model, GammaQuadrupletLoss(**LOSS_KW))
    model.fit(train_objectives=[(loader, lm)], epochs=2, warmup_steps=1, optimizer_params={"lr": 1e-3}, dropout=0,
              show_progress_bar=False)
    e1 = model.encode(texts)
    assert not np.allclose(e1, e0)
    out = str(tmp_path / "saved")
    model.save(out)
    pc = json.load(open(os.path.join(out, "1_Pooling", "config.json")))
    assert pc["pooling_mode_cls_token"] and not pc["pooling_mode_mean_tokens"] and pc["word_embedding_dimension"] == 64
    again = SentenceTransformer(out, device="cuda:0")
    assert again.cfg.pooling == "cls" and again.cfg.normalize
    np.testing.assert_array_equal(again.encode(texts), e1)
    out2 = str(tmp_path / "saved2")
    again.save(out2)
    assert json.load(open(os.path.join(out2, "1_Pooling", "config.json"))) == pc
