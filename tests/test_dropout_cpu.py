"""Dropout outside the fused kernels: the PyTorch compositions, BertMLM's gating, and the stream
counter in checkpoints."""
import pytest
import torch

from consensusml_amd import TrainConfig
from consensusml_amd.models.transformer import bert_tiny
from consensusml_amd.ops import transformer as T
from consensusml_amd.parallel.dist import DistInfo
from consensusml_amd.trainer.trainer import ConsensusTrainer


def test_compositions_eval_is_identity_train_drops():
    torch.manual_seed(0)
    x, r, w, b = torch.randn(5, 16), torch.randn(5, 16), torch.rand(16) + 0.5, torch.randn(16)
    qkv = torch.randn(2, 8, 3 * 2 * 8)
    for kw in (dict(dropout=0.5, training=False), dict(dropout=0.0)):
        assert all(torch.equal(a, c) for a, c in zip(T.add_norm(x, r, w, b, 1e-5, **kw),
                                                     T.add_norm(x, r, w, b, 1e-5)))
        assert torch.equal(T.norm(x, w, b, 1e-5, **kw), T.norm(x, w, b, 1e-5))
        assert torch.equal(T.fused_qkv_attention(qkv, 2, 8, **kw), T.fused_qkv_attention(qkv, 2, 8))
    s, _ = T.add_norm(x, r, w, b, 1e-5, dropout=0.5, rng=(3, 4))
    d = (s - x) / r                       # 0 where dropped, 1 / (1 - p) where kept
    assert set(d.round().unique().tolist()) == {0.0, 2.0}
    assert torch.equal(s, T.add_norm(x, r, w, b, 1e-5, dropout=0.5, rng=(3, 4))[0])
    y = T.norm(x, w, b, 1e-5, dropout=0.5, rng=(3, 4))
    assert 0 < (y == 0).sum() < y.numel()
    for kw in (dict(), dict(causal=True), dict(lens=torch.tensor([8, 5]))):
        o = T.fused_qkv_attention(qkv, 2, 8, dropout=0.5, rng=(3, 4), **kw)
        assert o.shape == (2, 8, 16) and not torch.equal(o, T.fused_qkv_attention(qkv, 2, 8, **kw))
    with pytest.raises(ValueError):
        T.norm(x, w, b, 1e-5, dropout=1.0)


def test_bert_tiny_dropout_gating():
    torch.manual_seed(1)
    m, m0 = bert_tiny(dropout=0.1, attn_dropout=0.1), bert_tiny()
    m0.load_state_dict(m.state_dict())
    ids = torch.randint(0, 510, (2, 32))
    a = m(ids)
    assert not torch.equal(a, m(ids))     # two train-mode forwards draw different masks
    a.float().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    assert torch.equal(m.eval()(ids), m0.eval()(ids))


def test_stream_counter_round_trips_through_checkpoint(tmp_path):
    cfg = TrainConfig()
    cfg.model.name, cfg.model.seq_len, cfg.model.dropout = "bert_tiny", 32, 0.1
    cfg.dtype, cfg.batch_per_worker, cfg.ckpt_dir = "fp32", 2, str(tmp_path / "ck")
    tr = ConsensusTrainer(cfg, info=DistInfo(0, 1, 0, torch.device("cpu"), "none"))
    tr.fit(2, log_every=0)
    saved = T.dropout_stream.state_dict()
    assert saved["counter"] == 2 * 7      # per step: the embedding + 2 layers x (attention + 2 norms)
    tr.save()
    tr.fit(3, log_every=0)
    assert T.dropout_stream.counter > saved["counter"]
    tr.load(cfg.ckpt_dir)
    assert T.dropout_stream.state_dict() == saved
