"""Partitioned whole-set inference (DistributedPCGNN.infer / infer_all / infer_global, pcg_infer_chunk_dist) on ONE GPU: two
and three ranks over gloo (collectives staged through the host) and one rank over RCCL, against FusedPCGNN.infer on the whole
graph with the same parameters - bit for bit, for whole shards, shuffled subsets with duplicates, an empty rank, many chunks of
differing counts, a shard no rank holds whole; the training state around a call is left exactly as it was.  -m gpu."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
NODES, B = 120000, 1024


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _reference(w, E, theta, dev):
    """FusedPCGNN on the whole graph with the partitioned run's parameters (same flat layout)"""
    from pcgnn_amd.handler import PCGNNTrainer
    fz = PCGNNTrainer(w, dict(engine="graph", seed=5, emb_size=E, batch_size=B), dev).fused
    fz.theta.copy_(theta)
    fz.params_changed()
    return fz


def _shuffled_with_dups(n, size, seed):
    rs = np.random.RandomState(seed)
    ids = np.concatenate([rs.choice(n, size, replace=False), rs.choice(n, size // 10)])
    rs.shuffle(ids)
    return ids


def _train(d, seed):
    """a window of two steps (no graphs: gloo) - theta moves, the second step's update is left pending"""
    ids = d.pick_epoch(2 * B, seed)
    d.train_window(ids, d.labels_of(ids), use_graphs=False)


def _worker(rank, world, E, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pcgnn_amd import synth, utils
        from pcgnn_amd.dist import DistributedPCGNN
        dev = torch.device("cuda", 0)
        w = synth.make_workload("t", NODES, 32, (20000, 100000, 400000), 0.15, seed=5, skew=1.5)
        cfg = dict(emb_size=E, rho=0.5, alpha=2.0, lr=0.01, weight_decay=0.001, batch_size=B, seed=11)
        d = DistributedPCGNN(w, cfg, dev, stage_host=True, window=2)
        twin = DistributedPCGNN(w, cfg, dev, stage_host=True, window=2) if world == 2 else None
        part = d.part
        for e in (d, twin) if twin is not None else (d,):
            _train(e, 0)
        assert int(d.opt_flag.item()) != 0, "an update is pending"

        # ---- every owned node, and the whole graph ----
        g, c = d.infer(None, want_center=True)
        fz = _reference(w, E, d.theta, dev)                  # (infer applied the pending update: theta is final now)
        rg, rc = fz.infer(torch.arange(part.lo, part.hi, dtype=torch.int32, device=dev), want_center=True)
        assert torch.equal(g, rg), "gnn logits of the owned nodes"
        assert torch.equal(c, rc), "centre logits of the owned nodes"
        ag, ac = d.infer_all(want_center=True)
        wg, wc = fz.infer(None, want_center=True)
        assert torch.equal(ag, wg) and torch.equal(ac, wc), "infer_all"
        assert torch.equal(d.infer(None), rg), "cached plan of the owned set"

        # ---- subsets: shuffled, duplicates, one rank with nothing; small chunks and a small halo: >= 4 chunks, counts differ ----
        sub = _shuffled_with_dups(part.n_local, 3000 if rank == 0 else 1200, seed=rank)
        if rank == 1:
            sub = sub[:0]
        sg, sc = d.infer(sub, chunk=600, want_center=True, halo_rows=1500)
        assert sg.shape == (len(sub), 2)
        if len(sub):
            rsg, rsc = fz.infer(torch.from_numpy(sub + part.lo).to(torch.int32).to(dev), want_center=True)
            assert torch.equal(sg, rsg) and torch.equal(sc, rsc), "subset with small chunks"
        assert rank != 0 or len(sub) > 4 * 600                # (rank 0: at least five chunks, the others fewer)

        # ---- evaluation: utils.test on the partitioned model = on the single-GPU engine with the same theta ----
        test_ids = np.setdiff1d(np.arange(w.n), w.idx_train)[::7]
        m_d = utils.test(test_ids, w.labels[test_ids], d, B, print_line=False)
        m_f = utils.test(test_ids, w.labels[test_ids], fz, B, print_line=False)
        assert m_d == m_f, (m_d, m_f)

        # ---- the training state is left alone: a call in the middle of a window ----
        if twin is not None:
            twin.flush()                                    # (d's calls above flushed: both start from no pending update)
            _train(d, 1)
            _train(twin, 1)
            win = {}
            for e in (d, twin):
                win[id(e)] = e.pick_epoch(B, 2)
                e.begin_window(win[id(e)])
            before = {k: getattr(d, k).clone() for k in ("s0_full", "row_gid")}
            before["halo_rows"] = d.halo.halo_rows.clone()
            before["req_out"] = d.halo.req_out.clone()
            before["data"] = d.data.clone()
            d.infer(None, chunk=5000)
            d.infer(sub, want_center=True, halo_rows=800)
            torch.cuda.synchronize()
            assert torch.equal(d.s0_full, before["s0_full"]) and torch.equal(d.row_gid, before["row_gid"])
            assert torch.equal(d.halo.halo_rows, before["halo_rows"]) and torch.equal(d.halo.req_out, before["req_out"])
            assert torch.equal(d.data, before["data"])
            for e in (d, twin):
                ids = win[id(e)]
                e.forward_sample(ids[:B // 2], e.labels_of(ids[:B // 2]), True, prefetch=False)
                _train(e, 3)
                e.flush()
            torch.cuda.synchronize()
            for name in ("theta", "m", "v", "step_counter", "s0_full"):
                assert torch.equal(getattr(d, name), getattr(twin, name)), name + " (with vs without infer)"
            d.check()
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _run(target, world, args, timeout):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world) + args + (port, q)) for r in range(world)]
    for p in procs:
        p.start()
    import queue
    import time
    res, deadline = [], time.time() + timeout
    try:
        while len(res) < len(procs):                          # (a worker that died without a result ends the wait)
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


@pytest.mark.parametrize("world,emb", [(2, 64), (3, 128)])
def test_ranks_infer_like_single_gpu(world, emb):
    _run(_worker, world, (emb,), 900)


def _worker_shard(rank, world, port, q):
    """synth.power_law_shard: no rank ever holds the whole graph; the reference is FusedPCGNN on the world-1 shard (= the
    whole graph, test_dist_cpu.py)"""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pcgnn_amd import synth
        from pcgnn_amd.dist import DistributedPCGNN
        dev = torch.device("cuda", 0)
        n, m, E = 200000, 4000000, 64
        sh = synth.power_law_shard(n, m, 3, world, rank)
        cfg = dict(emb_size=E, rho=0.5, alpha=2.0, lr=0.01, weight_decay=0.001, batch_size=B, seed=11)
        d = DistributedPCGNN(sh, cfg, dev, stage_host=True, window=2)
        _train(d, 0)
        g, c = d.infer(None, want_center=True)
        ag = d.infer_all()
        del sh
        full = synth.power_law_shard(n, m, 3, 1, 0)
        w = synth.Workload("full", full.X_local, full.labels_local.astype(np.int64), full.csr, np.ones(n, np.int64),
                           full.idx_train_local, list(full.train_pos))
        del full
        fz = _reference(w, E, d.theta, dev)
        part = d.part
        rg, rc = fz.infer(torch.arange(part.lo, part.hi, dtype=torch.int32, device=dev), want_center=True)
        assert torch.equal(g, rg) and torch.equal(c, rc), "owned nodes of a shard"
        assert torch.equal(ag, fz.infer()), "infer_all of a shard"
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_power_law_shard_world_2():
    _run(_worker_shard, 2, (), 900)


def _worker_w1(rank, world, port, q):
    """world size 1 over RCCL: an empty halo, the exchanges are copies"""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    d = None
    try:
        from pcgnn_amd import synth
        from pcgnn_amd.dist import DistributedPCGNN
        w = synth.make_workload("t", 40000, 32, (8000, 60000, 200000), 0.15, seed=5, skew=1.5)
        cfg = dict(emb_size=64, rho=0.5, alpha=2.0, lr=0.01, weight_decay=0.001, batch_size=256, seed=11)
        d = DistributedPCGNN(w, cfg, dev, window=4)
        ids = d.pick_epoch(4 * 256, 0)
        d.train_window(ids, d.labels_of(ids))
        g, c = d.infer(None, want_center=True)
        fz = _reference(w, 64, d.theta, dev)
        wg, wc = fz.infer(None, want_center=True)
        assert torch.equal(g, wg) and torch.equal(c, wc)
        assert torch.equal(d.infer_all(), wg)
        sub = _shuffled_with_dups(w.n, 5000, seed=3)
        assert torch.equal(d.infer(sub, chunk=1000), fz.infer(sub))
        d.check()
        q.put((0, "ok"))
    except Exception:  # pragma: no cover
        import traceback
        q.put((0, traceback.format_exc()))
    finally:
        if d is not None:
            d.close()
        dist.destroy_process_group()


def test_world_size_1_rccl():
    _run(_worker_w1, 1, (), 600)
