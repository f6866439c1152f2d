"""Worker-side momentum on the MI355X: the HIP kernel (csrc/kernels/worker_momentum.hip) against
a float64 oracle over its dispatch space (vector / scalar variant, tails, strided windows; with
a capped grid, workgroups that make several passes over their row with a partial last one), the
binding's argument checks, and the engine paths that only a
GPU reaches (bf16 rows, ``worker_batch()``, two ranks with overlapped bucket collectives)."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from test_dist_gloo import _cfg, _free_port

pytestmark = pytest.mark.gpu

CANARY = 12345.0     # fill of the buffers around a window (compared bit for bit with itself)


def _lengths():
    from consensusml_amd.ops import kernels as K
    # 1 .. 9: below, at and above one vector; 2047 .. 2049: around one wave-row of vectors;
    # PASS + 1: one element more than one workgroup covers in one pass (the grid grows with L, so
    # this is still one pass per workgroup: test_kernel_several_passes caps the grid)
    return [1, 7, 8, 9, 2047, 2048, 2049, K.WORKER_MOMENTUM_PASS + 1]


def _window(layout, R, L, dtype, dev):
    """(whole buffer, [R, L] window into it) filled with the canary."""
    if layout == "contiguous":
        buf = torch.full((64 + R * L + 64,), CANARY, dtype=dtype, device=dev)
        return buf, buf[64:64 + R * L].view(R, L)
    if layout == "window":      # a bucket's column range: offset and row stride multiples of 64
        W = 64 + -(-L // 64) * 64 + 64
        buf = torch.full((R, W), CANARY, dtype=dtype, device=dev)
        return buf, buf[:, 64:64 + L]
    W = L + 11                  # "odd": starts at an odd element, odd row stride -> scalar path
    buf = torch.full((R, W), CANARY, dtype=dtype, device=dev)
    return buf, buf[:, 3:3 + L]


@pytest.mark.parametrize("layout", ["contiguous", "window", "odd"])
@pytest.mark.parametrize("beta", [0.0, 0.9])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_kernel_float64_oracle(cuda, dtype, beta, layout):
    _oracle_cases(cuda, dtype, beta, layout, (1, 3, 8), _lengths(), 0)


@pytest.mark.parametrize("layout", ["window", "odd"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_kernel_several_passes(cuda, dtype, layout):
    """The launcher sizes the grid from L, so a workgroup makes a second pass only beyond 8192
    workgroups (millions of elements per row: the ResNet-50 / BERT rows at V = 8). ``grid_cap=1``
    leaves ONE workgroup per row at any R, so short rows exercise the same outer stride: with
    PASS = 8192 elements per pass, L = 2 PASS + 9 is two full passes, a third with one vector in
    it and a one-element tail on the vector variant ("window") and 17 passes, the last partial,
    on the scalar one ("odd"); L = 3 PASS + 1 is three full passes and a tail."""
    from consensusml_amd.ops import kernels as K
    P = K.WORKER_MOMENTUM_PASS
    _oracle_cases(cuda, dtype, 0.9, layout, (1, 3, 8), [2 * P + 9, 3 * P + 1], 1)


def _oracle_cases(cuda, dtype, beta, layout, Rs, Ls, grid_cap):
    """Same bound as the CPU test: |m' - (beta m + g)| <= 2^-23 (|beta m| + |g|) against float64
    (the kernel makes one fma rounding, <= 2^-24 |m'|), beta being the fp32 value the kernel
    multiplies with; the row must be the kernel's own state rounded to the row dtype."""
    from consensusml_amd.ops.native import lib
    gen = torch.Generator(device=cuda).manual_seed(11)
    b64 = float(torch.tensor(beta, dtype=torch.float32))
    for R in Rs:
        for L in Ls:
            rbuf, rows = _window(layout, R, L, dtype, cuda)
            mbuf, mom = _window(layout, R, L, torch.float32, cuda)
            if layout == "odd":
                assert rows.data_ptr() % 16 and mom.data_ptr() % 16
            mom.copy_(torch.randn(R, L, generator=gen, device=cuda))
            inside_r = torch.zeros_like(rbuf, dtype=torch.bool)
            inside_m = torch.zeros_like(mbuf, dtype=torch.bool)
            _window_like(inside_r, rows).fill_(True)
            _window_like(inside_m, mom).fill_(True)
            for _ in range(2):
                g = torch.randn(R, L, generator=gen, device=cuda).to(dtype)
                rows.copy_(g)
                r0, m0 = rbuf.clone(), mbuf.clone()
                before = mom.clone()
                lib().worker_momentum(rows, mom, beta, grid_cap=grid_cap)
                want = b64 * before.double() + g.double()
                bound = 2.0 ** -23 * ((b64 * before.double()).abs() + g.double().abs())
                err = (mom.double() - want).abs()
                assert bool((err <= bound).all()), (R, L, float((err - bound).max()))
                assert torch.equal(rows, mom.to(dtype)), (R, L)
                # canaries: every element outside the window is untouched, in both buffers
                assert torch.equal(rbuf[~inside_r], r0[~inside_r]), (R, L)
                assert torch.equal(mbuf[~inside_m], m0[~inside_m]), (R, L)


def _window_like(buf, win):
    """The view of ``buf`` with the geometry ``win`` has in its own buffer."""
    return torch.as_strided(buf, win.shape, win.stride(), win.storage_offset())


def test_kernel_nonfinite_propagates(cuda):
    from consensusml_amd.ops import kernels as K
    inf, nan = float("inf"), float("nan")
    rows = torch.tensor([[nan, inf, 1.0, -inf, 0.0, 1.0, 2.0, 3.0, 4.0]], device=cuda,
                        dtype=torch.bfloat16)
    mom = torch.tensor([[1.0, 1.0, inf, inf, nan, 1.0, 1.0, 1.0, 1.0]], device=cuda)
    K.worker_momentum(rows, mom, 0.5)
    m = mom[0].cpu()
    assert torch.isnan(m[0]) and m[1] == inf and m[2] == inf and torch.isnan(m[3])
    assert torch.isnan(m[4]) and m[5:].tolist() == [1.5, 2.5, 3.5, 4.5]
    assert torch.isnan(rows[0, 0]) and rows[0, 1] == inf and float(rows[0, 8]) == 4.5


def test_binding_rejects_bad_arguments(cuda):
    from consensusml_amd.ops.native import lib
    wm = lib().worker_momentum
    rows = torch.zeros(2, 64, dtype=torch.bfloat16, device=cuda)
    mom = torch.zeros(2, 64, device=cuda)
    wm(rows, mom, 0.9)
    with pytest.raises(RuntimeError, match="fp32"):
        wm(rows, mom.bfloat16(), 0.9)
    with pytest.raises(RuntimeError, match="bf16 or fp32"):
        wm(rows.half(), mom, 0.9)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        wm(rows, mom.cpu(), 0.9)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        wm(rows.cpu(), mom, 0.9)
    with pytest.raises(RuntimeError, match="shape"):
        wm(rows, mom[:, :63], 0.9)
    with pytest.raises(RuntimeError, match="shape"):
        wm(rows, mom[:1], 0.9)
    with pytest.raises(RuntimeError, match="2-D"):
        wm(rows[0], mom[0], 0.9)
    with pytest.raises(RuntimeError, match="unit column stride"):
        wm(torch.zeros(64, 2, dtype=torch.bfloat16, device=cuda).t(), mom, 0.9)
    with pytest.raises(RuntimeError, match="row strides"):
        wm(rows, torch.zeros(1, 64, device=cuda).expand(2, 64), 0.9)
    torch.cuda.synchronize()
    assert not rows.any() and not mom.any()


# ---------------------------------------------------------------------------- engine
def _spy(monkeypatch):
    from consensusml_amd.ops import kernels as K
    calls = []
    real = K.worker_momentum

    def spy(rows, mom, beta):
        g, m0 = rows.detach().clone(), mom.detach().clone()
        real(rows, mom, beta)
        calls.append((g.cpu(), m0.cpu(), mom.detach().cpu().clone(), rows.detach().cpu().clone(),
                      float(beta)))
    monkeypatch.setattr(K, "worker_momentum", spy)
    return calls


def _check_calls(calls, V, D, steps):
    """Each step made ONE [V, D] launch whose state is the update of the same captured rows:
    within one fp32 rounding (2^-24 |m'|, the kernel's single fma) of the float64 value, hence
    of the CPU reference op, which rounds twice (both are within 2^-23 (|beta m| + |g|) of the
    exact value, so within twice that of each other); the sent rows are that state in bf16."""
    from consensusml_amd.ops import reference as ref
    assert len(calls) == steps
    b64 = float(torch.tensor(0.9, dtype=torch.float32))
    for g, m0, m1, sent, beta in calls:
        assert g.shape == (V, D) and g.dtype == torch.bfloat16 and beta == 0.9
        exact = b64 * m0.double() + g.double()
        # (the float64 sum is itself rounded: 2^-53 of it, far inside the 2^-40 slack; 2^-126:
        # results in the subnormal range have an absolute, not a relative, half ulp)
        assert bool(((m1.double() - exact).abs()
                     <= (2.0 ** -24 + 2.0 ** -40) * exact.abs() + 2.0 ** -126).all())
        want, rows = m0.clone(), g.clone()
        ref.worker_momentum(rows, want, beta)
        bound = 2 * 2.0 ** -23 * ((beta * m0).abs() + g.float().abs())
        assert bool(((m1 - want).abs() <= bound).all())
        assert torch.equal(sent, m1.to(torch.bfloat16))
    for (_, _, m1, _, _), (_, m0, _, _, _) in zip(calls, calls[1:]):
        assert torch.equal(m1, m0)          # nothing else touches the state between steps


def test_engine_state_matches_reference(cuda, monkeypatch):
    from consensusml_amd import TrainConfig
    from consensusml_amd.parallel.dist import DistInfo
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    calls = _spy(monkeypatch)
    cfg = TrainConfig()
    cfg.dtype = "bf16"
    cfg.virtual_workers = 8
    cfg.agg.rule = "krum"
    cfg.agg.f = 2
    cfg.topology.kind = "sharded"
    cfg.topology.bucket_mb = 0.002
    cfg.optim.lr = 0.05
    cfg.optim.worker_momentum = True
    cfg.model.extra = {"classes": 10}
    tr = ConsensusTrainer(cfg, info=DistInfo(0, 1, 0, cuda, "none"))
    e = tr.engine
    assert e.s1 is None and e.wm.dtype == torch.float32
    tr.fit(3, log_every=0)
    torch.cuda.synchronize()
    _check_calls(calls, 8, e.flat.total, 3)
    assert torch.equal(e.wm.cpu(), calls[-1][2])
    assert calls[0][1].abs().sum() == 0 and calls[-1][2].abs().sum() > 0
    assert all(bool(torch.isfinite(p).all()) for p in tr.model.parameters())
    tr.close()


def _bert(batched, V, monkeypatch):
    from consensusml_amd import TrainConfig, perf
    from consensusml_amd.parallel.dist import DistInfo
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    cfg = TrainConfig()
    cfg.model.name = "bert_tiny"
    cfg.model.seq_len = 32
    cfg.batch_per_worker = 2
    cfg.virtual_workers = V
    cfg.agg.rule = "krum"
    cfg.agg.f = 1
    cfg.topology.kind = "sharded"
    cfg.optim.lr = 0.0          # same parameters on both paths at every step
    cfg.optim.worker_momentum = True
    cfg.seed = 5
    cfg.dtype = "bf16"
    pol = perf.policy().replace(batched_workers=batched)
    with monkeypatch.context() as mctx, perf.use_policy(pol):
        calls = _spy(mctx)
        tr = ConsensusTrainer(cfg, info=DistInfo(0, 1, 0, torch.device("cuda", 0), "none"))
        for _ in range(3):
            tr.train_step()
        torch.cuda.synchronize()
    D = tr.engine.flat.total
    wm = tr.engine.wm.cpu().clone()
    tr.close()
    return calls, wm, D


def test_engine_worker_batch_matches_sequential(cuda, monkeypatch):
    """``worker_batch()`` (one batched forward / backward, rows written by the ops) and the
    sequential loop each advance every row exactly once per step. Their gradient rows differ by
    bf16 GEMM rounding only (row-relative 2e-2, tests/test_batched_workers_gpu.py); the state
    is linear in them, so ||m_b - m_s|| <= 2e-2 sum_k beta^(t-k) ||g_k|| per row."""
    V, steps = 4, 3
    seq_calls, wm_s, D = _bert(False, V, monkeypatch)
    _check_calls(seq_calls, V, D, steps)
    bat_calls, wm_b, _ = _bert(True, V, monkeypatch)
    _check_calls(bat_calls, V, D, steps)
    budget = torch.zeros(V)
    for g, *_ in seq_calls:
        budget = 0.9 * budget + g.float().norm(dim=1)
    diff = (wm_b - wm_s).norm(dim=1)
    assert bool((wm_s.norm(dim=1) > 0).all())
    assert bool((diff <= 2e-2 * budget).all()), (diff.tolist(), budget.tolist())


# ---------------------------------------------------------------------------- two ranks, one GPU
def _rank_worker(rank, world, port, overlap, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from consensusml_amd.parallel import dist as D
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    D._INFO = None
    info = D.init_distributed("gloo", device="cuda:0")
    cfg = _cfg("krum", "sharded", 1, 0, 3)
    cfg.dtype = "bf16"
    cfg.topology.bucket_mb = 0.0002     # ~100 bf16 elements: four buckets for the MLP
    cfg.topology.overlap = overlap
    cfg.optim.momentum = 0.9
    cfg.optim.worker_momentum = True
    tr = ConsensusTrainer(cfg, info=info)
    tr.fit(3, log_every=0)
    torch.cuda.synchronize()
    torch.save({"params": [p.detach().cpu().clone() for p in tr.model.parameters()],
                "wm": tr.engine.wm.cpu().clone(), "overlap": tr.engine.overlap,
                "buckets": len(tr.engine.flat.buckets)},
               os.path.join(out_dir, f"o{int(overlap)}_{rank}.pt"))
    D.barrier()
    dist.destroy_process_group()


def test_gpu_two_ranks_overlap_bit_identical(cuda, tmp_path):
    """Per-bucket [1, L_b] launches in the flushes (overlap) against one [1, D] launch in step():
    bit-identical state and parameters, identical replicas."""
    world = 2
    for ov in (True, False):
        mp.spawn(_rank_worker, args=(world, _free_port(), ov, str(tmp_path)), nprocs=world,
                 join=True)
    for r in range(world):
        a = torch.load(tmp_path / f"o1_{r}.pt", weights_only=True)
        b = torch.load(tmp_path / f"o0_{r}.pt", weights_only=True)
        a0 = torch.load(tmp_path / "o1_0.pt", weights_only=True)
        assert a["overlap"] and not b["overlap"] and a["buckets"] >= 3
        assert a["wm"].abs().sum() > 0 and torch.equal(a["wm"], b["wm"])
        for x, y, z in zip(a["params"], b["params"], a0["params"]):
            assert torch.equal(x, y) and torch.equal(x, z)
