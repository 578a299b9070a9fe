"""Device-side evaluation counts (pcg_eval_counts) and what is built on them (ops.eval_counts, utils.device_metrics,
FusedPCGNN.evaluate, DistributedPCGNN.evaluate, utils.test / test_f1 with on_device=True) on the GPU: the integer vector ==
numpy's, bit-stable across runs and graph replays, and every metric == the host path's.  -m gpu."""
import os
import socket

import numpy as np
import pytest
import torch

from tests.eval_ref import counts_numpy, scores

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def device_counts(prob, y, th=None):
    from pcgnn_amd import ops
    status = ops.eval_status(dev())
    out = ops.eval_counts(torch.from_numpy(prob).to(dev()), torch.from_numpy(y.astype(np.int32)).to(dev()), th)
    got = out.cpu().numpy().view(np.uint64)
    assert int(status.item()) == 0, "status word"
    return got


def assert_counts(n, share, kind, T, seed):
    prob, y = scores(n, share, seed, kind)
    th = None if T == 100 else (np.array([0.37]) if T == 1 else np.linspace(0.0, 1.0, T))
    want = counts_numpy(prob, y, th)
    got = device_counts(prob, y, th)
    print(f"n {n} share {share} {kind} T {T}: tp fp fn tn n1 n0 2U = {got[:7].tolist()} (numpy {want[:7].tolist()})")
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"words that differ: {np.nonzero(got != want)[0][:10].tolist()}"


SMALL = [(n, share, kind, T) for n in (0, 1, 63, 64, 65, 1000) for share, kind, T in
         ((0.5, "continuous", 100), (0.145, "tied", 1), (0.9, "edges", 1024))]
MEDIUM = [(27573, share, kind, T) for share in (0.001, 0.01, 0.145, 0.5, 0.9) for kind, T in
          (("continuous", 100), ("tied", 1024), ("edges", 1))]
MEDIUM += [(200_000, 0.145, "tied", 100), (131_073, 0.5, "continuous", 100), (131_072, 0.5, "edges", 1024)]  # both sides of the one-workgroup sort
LARGE = [(2_000_000, 0.001, "continuous", 100), (2_000_000, 0.01, "tied", 1024), (2_000_000, 0.5, "continuous", 100),
         (2_000_000, 0.9, "edges", 1), (10_000_000, 0.01, "continuous", 100), (10_000_000, 0.5, "tied", 100),
         (10_000_000, 0.5, "continuous", 1024), (10_000_000, 0.9, "continuous", 1)]


@pytest.mark.parametrize("n,share,kind,T", SMALL + MEDIUM + LARGE)
def test_counts_equal_numpy(n, share, kind, T):
    assert_counts(n, share, kind, T, seed=n % 1000 + int(share * 1000) + T)


def test_all_scores_equal_and_one_class():
    prob, y = scores(70_000, 0.3, 3, "equal")
    assert np.array_equal(device_counts(prob, y), counts_numpy(prob, y))
    for yy in (np.zeros_like(y), np.ones_like(y)):
        assert np.array_equal(device_counts(prob, yy), counts_numpy(prob, yy))


@pytest.mark.parametrize("n,share", [(27573, 0.145), (400_000, 0.5)])
def test_graph_replay_and_repeat_are_bitwise(n, share):
    from pcgnn_amd import ops
    prob, y = scores(n, share, 11, "tied")
    p, l = torch.from_numpy(prob).to(dev()), torch.from_numpy(y).to(dev())
    eager = ops.eval_counts(p, l).clone()
    again = ops.eval_counts(p, l).clone()
    assert torch.equal(eager, again)
    assert np.array_equal(eager.cpu().numpy().view(np.uint64), counts_numpy(prob, y))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = ops.eval_counts(p, l)
    for _ in range(2):
        captured.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)
    assert int(ops.eval_status(dev()).item()) == 0


def test_bad_inputs_raise_through_the_status_bit():
    from pcgnn_amd import _lib, ops, utils as U
    prob, y = scores(5000, 0.2, 13)
    p = torch.from_numpy(prob).to(dev())
    assert U.device_metrics(p, y)["auc"] == U.roc_auc(y, prob[:, 1])
    bad = y.copy()
    bad[1234] = 2
    with pytest.raises(_lib.PcgnnLibraryError, match="label outside"):
        U.device_metrics(p, bad)
    assert int(ops.eval_status(dev()).item()) == 0               # (read and cleared)
    nan = prob.copy()
    nan[77, 1] = np.nan
    with pytest.raises(_lib.PcgnnLibraryError, match="NaN"):
        U.device_metrics(torch.from_numpy(nan).to(dev()), y)
    assert U.device_metrics(p, y)["auc"] == U.roc_auc(y, prob[:, 1])
    assert int(ops.eval_status(dev()).item()) == 0


def test_argument_errors_before_any_launch():
    from pcgnn_amd import _lib
    lib = _lib.load()
    assert lib.pcg_eval_workspace_bytes(-1, 100) == _lib.PCG_E_ARG
    assert lib.pcg_eval_workspace_bytes(10, 0) == _lib.PCG_E_ARG and lib.pcg_eval_workspace_bytes(10, 1025) == _lib.PCG_E_ARG
    assert lib.pcg_eval_workspace_bytes(1 << 31, 100) == _lib.PCG_E_ARG
    assert lib.pcg_eval_counts(None, None, 5, None, 100, None, None, None, None) == _lib.PCG_E_ARG


# ---- the engines ---------------------------------------------------------------------------------------------------------
def trainer(w, **cfg):
    from pcgnn_amd.handler import PCGNNTrainer
    return PCGNNTrainer(w, dict(engine="graph", seed=5, **cfg), dev())


def host_metrics(fz, ids, labels, B):
    from pcgnn_amd import utils as U
    prob = U.predict_proba(ids, fz, B)
    m = U.binary_metrics(labels, prob.argmax(axis=1), prob[:, 1])
    m["best_f1"], m["best_threshold"] = U.get_best_f1(labels, prob[:, 1])
    return m, prob


def check_engine(w, B, first_labeled, tmp_path):
    from pcgnn_amd import utils as U
    from pcgnn_amd.result_manager import ResultManager
    t = trainer(w, batch_size=B)
    for _ in range(3):
        t.run_epoch_one_graph()
    fz = t.fused
    ids = np.arange(first_labeled, w.n)
    held = ids[~np.isin(ids, w.idx_train)]
    for name, sel, lab in (("held-out", held, w.labels[held]), ("whole graph", None, w.labels)):
        want, prob = host_metrics(fz, np.arange(w.n) if sel is None else sel, lab, B)
        got = fz.evaluate(sel, lab)
        print(name, {k: got[k] for k in want})
        assert 0.0 < want["auc"] < 1.0 and len(np.unique(prob[:, 1])) > 100, "degenerate scores"
        for k, v in want.items():
            assert got[k] == v, (name, k, got[k], v)
    lab = w.labels[held]
    assert U.test(held, lab, fz, B, print_line=False, on_device=True) == U.test(held, lab, fz, B, print_line=False)
    valid = U.test_f1(held, lab, fz, B, flag="valid")
    assert U.test_f1(held, lab, fz, B, flag="valid", on_device=True) == valid
    assert U.test_f1(held, lab, fz, B, flag="test", valid_thresh=valid[4], on_device=True) == \
        U.test_f1(held, lab, fz, B, flag="test", valid_thresh=valid[4])
    lines = []
    for on_device in (False, True):
        rm = ResultManager(dict(model="PCGNN", data_name=w.name), root=str(tmp_path / f"res{int(on_device)}"))
        U.test(held, lab, fz, B, rm, epoch=3, epoch_best=2, flag="val", print_line=False, on_device=on_device)
        U.test(held, lab, fz, B, rm, epoch_best=2, flag="test", print_line=False, on_device=on_device)
        lines.append((open(rm.log_val_path).read().split("\n", 2)[2], open(rm.log_test_path).read().split("\n", 2)[2],
                      rm.df_val.to_dict(), rm.df_test[list(rm.df_val.columns[2:])].to_dict()))
    assert lines[0] == lines[1]
    assert "AUC-ROC" in lines[0][0] and "Test performance" in lines[0][1]
    fz.check()


def test_evaluate_yelp_like(tmp_path):
    from pcgnn_amd import synth
    check_engine(synth.yelp_like(0), 1024, 0, tmp_path)


def test_evaluate_amazon_like(tmp_path):
    from pcgnn_amd import synth
    check_engine(synth.amazon_like(0), 256, 3305, tmp_path)


def test_other_models_go_through_device_metrics():
    """a model without ``evaluate`` (here: an engine with a selection-list capacity of its own, evaluated batch by batch)"""
    from pcgnn_amd import synth, utils as U
    from pcgnn_amd.fused import FusedPCGNN
    w = synth.make_workload("mini", 6000, 32, (4000, 30000, 90000), 0.12, seed=3)
    t = trainer(w, batch_size=256)
    for _ in range(3):
        t.run_epoch_one_graph()
    fz = t.fused
    ids = np.setdiff1d(np.arange(w.n), w.idx_train)
    fz.eval_by_infer = False
    try:
        assert U.test(ids, w.labels[ids], fz, 256, print_line=False, on_device=True) == U.test(ids, w.labels[ids], fz, 256, print_line=False)
    finally:
        fz.eval_by_infer = True


# ---- partitioned ---------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, backend, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    d0 = torch.device("cuda", 0)
    if backend == "nccl":
        torch.cuda.set_device(d0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=d0)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    d = None
    try:
        from pcgnn_amd import synth, utils as U
        from pcgnn_amd.dist import DistributedPCGNN
        w = synth.make_workload("t", 40000, 32, (8000, 60000, 200000), 0.15, seed=5, skew=1.5)
        cfg = dict(emb_size=64, rho=0.5, alpha=2.0, lr=0.01, weight_decay=0.001, batch_size=256, seed=11)
        d = DistributedPCGNN(w, cfg, d0, stage_host=backend == "gloo", window=2)
        for e in range(3):
            ids = d.pick_epoch(2 * 256, e)
            d.train_window(ids, d.labels_of(ids), **({} if backend == "nccl" else dict(use_graphs=False)))
        test_ids = np.setdiff1d(np.arange(w.n), w.idx_train)[::3]
        lab = w.labels[test_ids]
        prob = U.predict_proba(test_ids, d, 256)
        want = U.binary_metrics(lab, prob.argmax(axis=1), prob[:, 1])
        want["best_f1"], want["best_threshold"] = U.get_best_f1(lab, prob[:, 1])
        got = d.evaluate(test_ids, lab)
        for k, v in want.items():
            assert got[k] == v, (k, got[k], v)
        assert U.test(test_ids, lab, d, 256, print_line=False, on_device=True) == U.test(test_ids, lab, d, 256, print_line=False)
        d.check()
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        if d is not None and backend == "nccl":
            d.close()
        dist.destroy_process_group()


def _run(world, backend, timeout):
    import queue
    import time
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, backend, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res, deadline = [], time.time() + timeout
    try:
        while len(res) < len(procs):                          # (a worker that died without a result ends the wait: no retry)
            try:
                res.append(q.get(timeout=5))
            except queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not dead and time.time() < deadline, f"workers ended without a result: exit codes {dead}"
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for rank, msg in res:
        assert msg == "ok", f"rank {rank}: {msg}"


def test_distributed_evaluate_world_1_rccl():
    _run(1, "nccl", 600)


def test_distributed_evaluate_world_2_gloo():
    _run(2, "gloo", 600)
