"""The whole-epoch engine's host state machine (FusedPCGNN.stage_epoch / take_prefetched / plan_staged / epoch_run and the two
epoch buffer sets) when the epoch shape changes on ONE engine: another number of epochs per group, another batch size, a batch
above max_batch, with a set prepared ahead (prefetch=True / "stream") and with a deferred update pending.

Every scenario is compared bit for bit (theta, Adam moments, step counter) with a trainer that starts from the same
parameters and runs the SAME epoch numbers one at a time, each as one plain ``run_epoch_one_graph()`` - the path
tests/test_gpu_parity.py ties to eager ``train_step``.  Which epoch numbers a group trained is asserted, not inferred: its
staged ids are compared with the stand-alone sampler at exactly those numbers.

The rule under test for a set prepared ahead and then dropped (FusedPCGNN.stage_epoch): its epoch numbers are skipped.

Run with ``pytest -m gpu`` on an MI355X."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

STATE = ("theta", "m", "v", "step_counter")
BATCH = 256


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def env():
    import pcgnn_amd  # noqa: F401
    from pcgnn_amd import synth
    from pcgnn_amd.handler import PCGNNTrainer
    w = synth.make_workload("mini", 6000, 32, (4000, 30000, 90000), 0.12, seed=3)
    first = PCGNNTrainer(w, dict(engine="graph", batch_size=BATCH, seed=5), dev())
    n, nb = first.pick_size, first.batches_per_epoch()
    assert n % BATCH != 0 and nb >= 3                    # every epoch's last batch is the shorter one
    return SimpleNamespace(w=w, Trainer=PCGNNTrainer, theta0=first.fused.theta.clone(), n=n, nb=nb, sampler=first.sampler,
                           labels=first.labels_i32, refs={}, ids={})


def new_trainer(env, batch_size=BATCH):
    t = env.Trainer(env.w, dict(engine="graph", batch_size=batch_size, seed=5), dev())
    t.fused.theta.copy_(env.theta0)
    t.fused.params_changed()
    return t


def sampled(env, epochs):
    """the shuffled picks of the given epoch numbers from the stand-alone sampler, epoch by epoch (computed once per number)"""
    for e in epochs:
        if e not in env.ids:
            env.ids[e] = env.sampler.pick_shuffled(env.n, torch.empty(env.n, dtype=torch.int32, device=dev()), epoch=e)
    return torch.cat([env.ids[e] for e in epochs])


def counter(t) -> int:
    return int(t._epoch_dev[0].item())


def one_by_one(t, epochs, tail=None):
    """the given epoch numbers one at a time, each a plain whole-epoch launch (+ tail = (epoch number, n_steps): the first
    n_steps batches of one more)"""
    for e in epochs:
        t._epoch_dev[0] = e
        t.run_epoch_one_graph()
    if tail is not None:
        t._epoch_dev[0] = tail[0]
        t.run_epoch_one_graph(n_steps=tail[1])


def snapshot(t):
    torch.cuda.synchronize()
    t.fused.check()
    return {name: getattr(t.fused, name).clone() for name in STATE}


def reference(env, epochs, tail=None):
    """what a fresh trainer holds after ``one_by_one`` (computed once per sequence, shared, left unchanged)"""
    key = (tuple(epochs), tail)
    if key not in env.refs:
        t = new_trainer(env)
        one_by_one(t, epochs, tail)
        env.refs[key] = snapshot(t)
        assert int(env.refs[key]["step_counter"].item()) == len(epochs) * env.nb + (tail[1] if tail else 0)
    return env.refs[key]


def assert_equals(t, ref, what=""):
    got = snapshot(t)
    for name in STATE:
        assert torch.equal(got[name], ref[name]), f"{name} {what}"
    assert torch.isfinite(got["theta"]).all()


def run_group(env, t, epochs, prefetch=False, **kw):
    """one group of len(epochs) epochs as one launch; asserts that the group trained exactly the given epoch numbers, that the
    set prepared ahead (prefetch) holds the numbers after them, and where the device epoch counter stands"""
    k, n, f = len(epochs), env.n, t.fused
    assert t.run_epoch_one_graph(prefetch=prefetch, n_epochs=k, **kw) == k * n
    torch.cuda.synchronize()
    trained = f._ep_sets[f._cur ^ 1 if prefetch else f._cur]["ids"][:k * n]
    assert torch.equal(trained, sampled(env, epochs)), f"the group trained other epochs than {list(epochs)}"
    if prefetch:
        ahead = list(range(epochs[-1] + 1, epochs[-1] + 1 + k))
        assert f._cur_ready and torch.equal(f._ep_ids[:k * n], sampled(env, ahead))
        assert counter(t) == ahead[-1] + 1
    else:
        assert not f._cur_ready and counter(t) == epochs[-1] + 1


def stage_and_check_dropped(t, k):
    """The shape-changing stage_epoch on an engine that holds a prepared set: the set is dropped BEFORE anything is replayed
    (replaying it would run the steps over zeroed plan slots and ids laid out for the old shape)."""
    f = t.fused
    assert f._cur_ready
    f.stage_epoch(t.pick_size, t.batch_size, k)
    assert not f._cur_ready and getattr(f, "_ev_ready", None) is None


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [(4, 2), (2, 4)], ids=["4_then_2", "2_then_4"])
@pytest.mark.parametrize("then", ["prefetch", "plain", "staged"])
@pytest.mark.parametrize("p", [True, "stream"], ids=["fork", "stream"])
def test_prepared_set_then_another_group_size(env, p, then, order):
    """A group of k1 epochs with the next k1 prepared ahead, then a group of k2: the prepared set is dropped and its epoch
    numbers k1 .. 2 k1 - 1 are skipped - the second group trains 2 k1 .. 2 k1 + k2 - 1, sampled and planned at the new shape -
    whether it runs with a set prepared ahead again, as a plain group, or staged and stepped batch by batch.  4 then 2 stays
    inside the buffers (the shape-change branch of stage_epoch), 2 then 4 re-allocates them; the first group's last update is
    pending across the change."""
    k1, k2 = order
    t = new_trainer(env)
    f = t.fused
    first, second = list(range(k1)), list(range(2 * k1, 2 * k1 + k2))
    run_group(env, t, first, prefetch=p, flush=False)
    stage_and_check_dropped(t, k2)
    assert counter(t) == 2 * k1
    if then == "prefetch":
        run_group(env, t, second, prefetch=p)
    elif then == "plain":
        run_group(env, t, second)
    else:
        ids = t.start_epoch_staged(k2)
        torch.cuda.synchronize()
        assert torch.equal(ids, sampled(env, second)) and counter(t) == 2 * k1 + k2 and not f._cur_ready
        for b in range(k2 * env.nb):
            f.epoch_step(b, defer=True)
    f.flush()
    assert_equals(t, reference(env, first + second), f"({k1} epochs prepared ahead, then {k2}: {then})")


@pytest.mark.parametrize("p", [True, "stream"], ids=["fork", "stream"])
def test_prepared_set_same_shape_flush_flips_on_the_last_call(env, p):
    """Three single epochs, each preparing the next, the last one with the end-of-epoch flush (another graph key: a capture
    with a prepared set at hand, whose warm-up plans and runs that set): epochs 0, 1, 2, nothing skipped, epoch 3 ready."""
    t = new_trainer(env)
    run_group(env, t, [0], prefetch=p, flush=False)
    run_group(env, t, [1], prefetch=p, flush=False)
    run_group(env, t, [2], prefetch=p, flush=True)
    assert_equals(t, reference(env, [0, 1, 2]))
    assert counter(t) == 4 and t.fused._cur_ready


def test_alternating_groups_of_four_and_one(env):
    """ModelHandler.train with valid_epochs = 5: groups of 4, 1, 4, 1 epochs on one engine, the last update of each left
    pending (flush=False) across the shape change: ten consecutive epochs, the counter at 10."""
    t = new_trainer(env)
    for group in ([0, 1, 2, 3], [4], [5, 6, 7, 8], [9]):
        run_group(env, t, group, flush=False)
    t.fused.flush()
    assert_equals(t, reference(env, list(range(10))))
    assert counter(t) == 10


def test_same_shape_again_after_a_detour_and_a_group_cut_short(env):
    """4, 2, 4, 2 epochs - a shape seen before comes back after another one: its graphs are captured again (or reused) over
    slots that were zeroed in between - and then, directly after a shape change, a group of 4 cut short two batches into its
    third epoch: epochs 0 .. 13 and the first two batches of epoch 14; the cut group's four epochs 12 .. 15 were all sampled."""
    t = new_trainer(env)
    n, nb, f = env.n, env.nb, t.fused
    for group in ([0, 1, 2, 3], [4, 5], [6, 7, 8, 9], [10, 11]):
        run_group(env, t, group, flush=False)
    r = 2 * nb + 2
    assert t.run_epoch_one_graph(n_steps=r, n_epochs=4) == 2 * n + 2 * BATCH
    torch.cuda.synchronize()
    assert torch.equal(f._ep_ids[:4 * n], sampled(env, [12, 13, 14, 15])) and counter(t) == 16
    assert_equals(t, reference(env, list(range(14)), tail=(14, 2)))
    assert int(f.step_counter.item()) == 12 * nb + r


def test_another_batch_size_on_one_trainer(env):
    """batch 256 -> 128 (a smaller plan stride: the epoch buffers are re-allocated) -> 512 (above max_batch: every buffer of
    the engine is), two epochs each, each change made with the group's last update pending.  Reference: a fresh trainer per
    batch size, built for it, that runs its two epochs one by one from the state the one before left."""
    t = new_trainer(env)
    f = t.fused
    refs = {bs: new_trainer(env, bs) for bs in (BATCH, 128, 512)}
    before = None
    for bs, group in ((BATCH, [0, 1]), (128, [2, 3]), (512, [4, 5])):
        t.batch_size = bs
        if bs == 512:
            assert bs > f.maxB
        run_group(env, t, group, flush=False)
        assert f._ep_shape == (env.n, bs, 2) and len(f._ep_batches) == 2 * -(-env.n // bs) and f.maxB == max(BATCH, bs)
        r = refs[bs]
        if before is not None:
            before.fused.flush()
            for name in STATE:
                getattr(r.fused, name).copy_(getattr(before.fused, name))
            r.fused.params_changed()
        one_by_one(r, group)
        before = r
    f.flush()
    assert_equals(t, snapshot(before))
    assert counter(t) == 6 and int(f.step_counter.item()) == 2 * sum(-(-env.n // bs) for bs in (BATCH, 128, 512))


@pytest.mark.parametrize("explicit_n", ["pick_size", 300])
@pytest.mark.parametrize("p", [True, "stream"], ids=["fork", "stream"])
def test_prepared_set_then_other_public_calls(env, p, explicit_n):
    """What the other public calls do to a set prepared ahead.

    train_step on an ad-hoc batch (within max_batch), infer() and chosen() leave the epoch buffers alone: the set stays ready
    and start_epoch_staged() afterwards starts on the prepared epoch - nothing is sampled, the counter does not move.

    begin_epoch MUST invalidate it: it stages the caller's ids in the current set - the prepared one - (same shape), or changes
    the shape (another n).  Either way the set is dropped, its epoch number is skipped and start_epoch_staged() afterwards
    samples the next one.

    The parameters equal a trainer's that made the same calls and never prepared anything ahead."""
    n, nb = env.n, env.nb
    t, r = new_trainer(env), new_trainer(env)
    adhoc = env.sampler.pick(100, 999)
    adhoc_lab = env.labels[adhoc.long()]
    m = n if explicit_n == "pick_size" else explicit_n
    own = env.sampler.pick(m, 77)
    own_lab = env.labels[own.long()]
    some = torch.arange(0, 500, 7, dtype=torch.int32, device=dev())

    def other_calls(x):
        x.fused.train_step(adhoc, adhoc_lab)
        logits = x.fused.infer()
        ch = x.fused.chosen(some)
        return logits, ch.ids.clone(), ch.dist.clone()

    def own_epoch(x):
        x.fused.begin_epoch(own, own_lab, BATCH)
        for b in range(-(-m // BATCH)):
            x.fused.epoch_step(b)

    f = t.fused
    run_group(env, t, [0], prefetch=p, flush=False)                 # epoch 1 is prepared
    out_t = other_calls(t)
    assert f._cur_ready and counter(t) == 2
    ids = t.start_epoch_staged()
    torch.cuda.synchronize()
    assert not f._cur_ready and counter(t) == 2 and torch.equal(ids, sampled(env, [1]))
    for b in range(nb):
        f.epoch_step(b, defer=True)
    run_group(env, t, [2], prefetch=p, flush=False)                 # epoch 3 is prepared ...
    own_epoch(t)                                                      # ... and dropped
    assert not f._cur_ready and getattr(f, "_ev_ready", None) is None and counter(t) == 4
    ids = t.start_epoch_staged()
    torch.cuda.synchronize()
    assert counter(t) == 5 and torch.equal(ids, sampled(env, [4]))
    for b in range(nb):
        f.epoch_step(b, defer=True)
    f.flush()

    one_by_one(r, [0])
    out_r = other_calls(r)
    one_by_one(r, [1, 2])
    own_epoch(r)
    one_by_one(r, [4])
    assert_equals(t, snapshot(r))
    for a, b in zip(out_t, out_r):
        assert torch.equal(a, b)
