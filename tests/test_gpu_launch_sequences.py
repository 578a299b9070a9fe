"""The order of the library calls the engine enqueues for a fixed script of public calls (FusedPCGNN's eager calls,
train_step_graph, the staged-epoch calls, PCGNNTrainer.run_epoch_one_graph / FusedPCGNN.epoch_run), compared with sequences
written out below.

The sequences are a RECORD: they were taken with this module's recorder from the commit before the staged-epoch engine moved
to epoch.py (there this file passes unedited).  A restructuring of the host code that keeps every launch, and the order of the
launches, leaves them as they are; a change that is meant to add, drop or reorder a launch edits the sequence it changes.

Recorder: ``pcgnn_amd._lib.check`` is replaced by a wrapper that notes its second argument - the entry point's name - and calls
through.  Every launch of fused.py, epoch.py, ops.py and wholeset.py passes through ``_lib.check(lib.<entry>(...), "<entry>")``,
looked up as a module attribute at the time of the call.  A capture's warm-up and the capture itself enqueue (and are recorded);
a graph replay enqueues nothing.

Every script runs twice, on two fresh engines with the same parameters: once recorded, once not.  The two end bit for bit
equal (theta, Adam moments, step counter) - the recorder changes nothing - and raise no status bit.

Workload: tests/test_gpu_epoch_engine.py's (6000 nodes, three relations, batch 256): three batches per epoch, the last one
short - the smallest at which the short last batch, the two buffer sets and the three-step minimum of the classifier-ahead
sequence all occur.

Run with ``pytest -m gpu`` on an MI355X."""
import math
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
    return make_env()


def make_env():
    import pcgnn_amd  # noqa: F401
    from pcgnn_amd import synth
    from pcgnn_amd.handler import PCGNNTrainer
    w = synth.make_workload("mini", 6000, 32, (4000, 30000, 90000), 0.12, seed=3)
    first = PCGNNTrainer(w, dict(engine="graph", batch_size=BATCH, seed=5), dev())
    n, nb = first.pick_size, first.batches_per_epoch()
    assert n % BATCH != 0 and nb >= 3                    # every epoch's last batch is the shorter one
    return SimpleNamespace(w=w, Trainer=PCGNNTrainer, theta0=first.fused.theta.clone(), n=n, nb=nb)


def new_trainer(env, pipeline=None, ahead=None):
    """pipeline / ahead: the engine's two switches, set as tests/test_gpu_pipelined_step.py and tests/test_gpu_clf_ahead.py set
    them (None: the engine's default)"""
    t = env.Trainer(env.w, dict(engine="graph", batch_size=BATCH, seed=5), dev())
    t.fused.theta.copy_(env.theta0)
    t.fused.params_changed()
    if pipeline is not None:
        t.fused.pipeline = pipeline
    if ahead is not None:
        t.fused.clf_ahead = ahead
    return t


def timed(f, call):
    """a call that must append exactly one (start, end) pair to ``_prof``, with a finite, non-negative time between the two"""
    def run():
        before = len(f._prof)
        call()
        assert len(f._prof) == before + 1, "a timed call appends exactly one event pair"
        start, end = f._prof[-1]
        torch.cuda.synchronize()
        ms = start.elapsed_time(end)
        assert math.isfinite(ms) and ms >= 0.0
    return run


def batch(t, size, epoch):
    ids = t.sampler.pick(size, epoch)
    return ids, t.labels_i32[ids.long()]


# -- the scripts: generators of (label, call); what a script enqueues before its first label (its inputs) is not compared -----
def eager_script(t):
    import torch.nn.functional as nnf
    f = t.fused
    ids, lab = batch(t, 200, 999)
    big, big_lab = batch(t, f.maxB + 16, 998)
    bigger, bigger_lab = batch(t, f.maxB + 48, 997)

    def forward_backward():
        gnn, center = f.forward(ids, lab)
        (nnf.cross_entropy(gnn, lab.long()) + 2.0 * nnf.cross_entropy(center, lab.long())).backward()

    def custom():
        f.train_step_custom(ids, lab, lambda gnn, center, y: nnf.cross_entropy(gnn, y.long()) + 2.0 * nnf.cross_entropy(center, y.long()))

    yield "train_step", lambda: f.train_step(ids, lab)
    yield "train_step(defer)", lambda: f.train_step(ids, lab, defer=True)
    yield "flush", f.flush
    yield "predict", lambda: f.predict(ids)
    yield "gradients(acts)", lambda: f.gradients(ids, lab, via="acts")
    yield "gradients(slabs)", lambda: f.gradients(ids, lab, via="slabs")
    yield "forward+backward", forward_backward
    yield "train_step_custom", custom
    yield "train_step(max_batch+16)", lambda: f.train_step(big, big_lab)          # the grow path: ONE flush in front
    assert f.maxB == BATCH + 16
    yield "predict(above max_batch)", lambda: f.predict(bigger)
    assert f.maxB == BATCH + 48


def step_graph_script(t):
    f = t.fused
    ids, lab = batch(t, 200, 999)
    yield "first", lambda: f.train_step_graph(ids, lab)
    yield "second", lambda: f.train_step_graph(ids, lab)
    f._prof = []
    yield "timed", timed(f, lambda: f.train_step_graph(ids, lab, timed=True))
    f._prof = None


def epoch_step_script(t):
    f = t.fused
    ids = t.start_epoch(0)
    lab = t.labels_i32[ids.long()]
    nb = t.batches_per_epoch()
    yield "begin_epoch", lambda: f.begin_epoch(ids, lab, BATCH)
    for b in range(nb):
        yield f"epoch_step({b}) first", lambda b=b: f.epoch_step(b)
    for b in range(nb):
        yield f"epoch_step({b}) replay", lambda b=b: f.epoch_step(b)
    yield "epoch_step(0, defer) first", lambda: f.epoch_step(0, defer=True)
    yield "epoch_step(0, defer) replay", lambda: f.epoch_step(0, defer=True)
    f._prof = []
    yield "epoch_step_timed(0, eager)", timed(f, lambda: f.epoch_step_timed(0, eager=True))
    yield "epoch_step_timed(0, graphs) first", timed(f, lambda: f.epoch_step_timed(0, eager=False))
    yield "epoch_step_timed(0, graphs) again", timed(f, lambda: f.epoch_step_timed(0, eager=False))
    f._prof = None
    yield "flush", f.flush


def epoch_run_script(**kw):
    repeat = kw.pop("repeat")

    def script(t):
        for i in range(repeat):
            yield f"call {i}", lambda: t.run_epoch_one_graph(**kw)
    return script


def rest_of_epoch_script(t):
    f = t.fused
    yield "start_epoch_staged", t.start_epoch_staged
    yield "epoch_step(0, defer)", lambda: f.epoch_step(0, defer=True)
    yield "epoch_run(first_step=1)", lambda: f.epoch_run(first_step=1)


EPOCH_RUNS = {
    "plain": epoch_run_script(repeat=2),
    "n_steps=2": epoch_run_script(repeat=1, n_steps=2),
    "n_epochs=2": epoch_run_script(repeat=1, n_epochs=2),
    "prefetch": epoch_run_script(repeat=3, prefetch=True),
    "stream": epoch_run_script(repeat=3, prefetch="stream"),
    "first_step=1": rest_of_epoch_script,
}
# pipeline, clf_ahead
MODES = {"serial": (False, None), "pipelined": (True, False), "pipelined_ahead": (True, True)}


def record(script, t, log):
    """-> [(label, the entry points the call enqueued)]; log: the list the recorder appends to (stays empty without one)"""
    out = []
    for label, call in script(t):
        mark = len(log)
        call()
        out.append((label, " ".join(log[mark:])))
    return out


def recorded(monkeypatch, script, t):
    from pcgnn_amd import _lib
    log, real = [], _lib.check

    def check(rc, what):
        log.append(what)
        return real(rc, what)

    with monkeypatch.context() as m:
        m.setattr(_lib, "check", check)
        return record(script, t, log)


def snapshot(t):
    torch.cuda.synchronize()
    t.fused.check()
    return {name: getattr(t.fused, name).clone() for name in STATE}


def run_case(env, monkeypatch, case, script, pipeline=None, ahead=None):
    a, b = new_trainer(env, pipeline, ahead), new_trainer(env, pipeline, ahead)
    got = recorded(monkeypatch, script, a)
    plain = record(script, b, [])
    assert [label for label, _ in plain] == [label for label, _ in got]
    sa, sb = snapshot(a), snapshot(b)
    for name in STATE:
        assert torch.equal(sa[name], sb[name]), f"{name}: the recorded run and the plain one differ ({case})"
    assert torch.isfinite(sa["theta"]).all() and int(sa["step_counter"].item()) > 0
    want = EXPECTED[case]
    assert [label for label, _ in got] == [label for label, _ in want]
    for (label, seq), (_, exp) in zip(got, want):
        assert seq.split() == exp.split(), f"{case}: {label}"
    return a


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [False, True], ids=["serial", "pipelined"])
def test_eager_calls(env, monkeypatch, pipeline):
    """no eager call's launches depend on the pipeline switch: one record for both"""
    run_case(env, monkeypatch, "eager", eager_script, pipeline)


def test_train_step_graph(env, monkeypatch):
    run_case(env, monkeypatch, "train_step_graph", step_graph_script)
    assert EXPECTED["train_step_graph"][1] == ("second", "")


def test_staged_epoch_step_by_step(env, monkeypatch):
    run_case(env, monkeypatch, "epoch_step", epoch_step_script)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("what", list(EPOCH_RUNS))
def test_epoch_run(env, monkeypatch, what, mode):
    pipeline, ahead = MODES[mode]
    t = run_case(env, monkeypatch, f"{what}/{mode}", EPOCH_RUNS[what], pipeline, ahead)
    assert not t.fused.touched_on
    launches = " ".join(seq for _, seq in EXPECTED[f"{what}/{mode}"]).split()
    # (the mode decides the schedule at this shape - n_steps=2 and the two batches after first_step=1 are too short a sequence
    #  for the classifier to run two batches ahead)
    assert ("pcg_dense_select_train" in launches or "pcg_dense_select_ahead" in launches) == pipeline
    assert ("pcg_dense_select_ahead" in launches) == (bool(ahead) and what not in ("n_steps=2", "first_step=1"))


@pytest.mark.parametrize("what", ["plain", "prefetch"])
def test_epoch_run_touched_rows(env, monkeypatch, what):
    monkeypatch.setenv("PCG_TOUCHED", "1")
    t = run_case(env, monkeypatch, f"{what}/touched", EPOCH_RUNS[what])
    assert t.fused.touched_on


# -- the record ----------------------------------------------------------------------------------------------------------
EXPECTED = {
    'eager': [
        ('train_step', 'pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_gather_train pcg_train_dense pcg_adam_flush'),
        ('train_step(defer)', 'pcg_plan_epochs pcg_choose_gather_train pcg_train_dense'),
        ('flush', 'pcg_adam_flush'),
        ('predict', 'pcg_adam_flush pcg_plan_epochs pcg_score_table pcg_choose_gather_planned pcg_train_dense'),
        ('gradients(acts)', 'pcg_adam_flush pcg_plan_epochs pcg_score_table pcg_pos_sort pcg_choose_gather_planned pcg_train_dense pcg_wgrad'),
        ('gradients(slabs)',
         'pcg_adam_flush pcg_plan_epochs pcg_score_table pcg_pos_sort pcg_choose_gather_planned pcg_train_dense '
         'pcg_adam_step'),
        ('forward+backward',
         'pcg_adam_flush pcg_plan_epochs pcg_score_table pcg_pos_sort pcg_choose_gather_planned pcg_train_dense '
         'pcg_dense_vjp pcg_wgrad'),
        ('train_step_custom',
         'pcg_adam_flush pcg_plan_epochs pcg_score_table pcg_pos_sort pcg_choose_gather_planned pcg_train_dense '
         'pcg_dense_vjp pcg_wgrad'),
        ('train_step(max_batch+16)',
         'pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_gather_train pcg_train_dense '
         'pcg_adam_flush'),
        ('predict(above max_batch)', 'pcg_adam_flush pcg_plan_epochs pcg_score_table pcg_choose_gather_planned pcg_train_dense'),
    ],
    'train_step_graph': [
        ('first',
         'pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_gather_train pcg_train_dense '
         'pcg_adam_flush pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_gather_train '
         'pcg_train_dense pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_gather_train '
         'pcg_train_dense pcg_adam_flush'),
        ('second', ''),
        ('timed', ''),
    ],
    'epoch_step': [
        ('begin_epoch', 'pcg_plan_epochs'),
        ('epoch_step(0) first',
         'pcg_adam_flush pcg_step_scores pcg_pos_sort pcg_choose_gather_train pcg_train_dense pcg_adam_flush '
         'pcg_adam_flush pcg_choose_gather_train pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
        ('epoch_step(1) first',
         'pcg_adam_flush pcg_choose_gather_train pcg_train_dense pcg_adam_flush pcg_adam_flush pcg_choose_gather_train '
         'pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
        ('epoch_step(2) first',
         'pcg_adam_flush pcg_choose_gather_train pcg_train_dense pcg_adam_flush pcg_adam_flush pcg_choose_gather_train '
         'pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
        ('epoch_step(0) replay', ''),
        ('epoch_step(1) replay', ''),
        ('epoch_step(2) replay', ''),
        ('epoch_step(0, defer) first',
         'pcg_adam_flush pcg_choose_gather_train pcg_train_dense pcg_adam_flush pcg_choose_gather_train pcg_train_dense '
         'pcg_step_scores pcg_pos_sort'),
        ('epoch_step(0, defer) replay', ''),
        ('epoch_step_timed(0, eager)', 'pcg_choose_gather_train pcg_train_dense'),
        ('epoch_step_timed(0, graphs) first',
         'pcg_adam_flush pcg_step_scores pcg_pos_sort pcg_choose_gather_train pcg_train_dense pcg_adam_flush '
         'pcg_choose_gather_train pcg_train_dense pcg_step_scores pcg_pos_sort'),
        ('epoch_step_timed(0, graphs) again', ''),
        ('flush', 'pcg_adam_flush'),
    ],
    'plain/serial': [
        ('call 0',
         'pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_gather_train pcg_train_dense '
         'pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush pcg_adam_flush '
         'pcg_pick_shuffled_epochs pcg_plan_epochs pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train '
         'pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
        ('call 1', ''),
    ],
    'plain/pipelined': [
        ('call 0',
         'pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_train_part pcg_choose_train_part '
         'pcg_dense_select_train pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part pcg_train_dense '
         'pcg_adam_flush pcg_adam_flush pcg_pick_shuffled_epochs pcg_plan_epochs pcg_choose_train_part '
         'pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part '
         'pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
        ('call 1', ''),
    ],
    'plain/pipelined_ahead': [
        ('call 0',
         'pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_train_part pcg_step_scores pcg_pos_sort '
         'pcg_clf_step pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_dense_select_ahead '
         'pcg_choose_train_part pcg_train_dense pcg_adam_flush pcg_adam_flush pcg_pick_shuffled_epochs pcg_plan_epochs '
         'pcg_choose_train_part pcg_step_scores pcg_pos_sort pcg_clf_step pcg_choose_train_part pcg_dense_select_ahead '
         'pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_train_dense pcg_adam_flush '
         'pcg_step_scores pcg_pos_sort'),
        ('call 1', ''),
    ],
    'n_steps=2/serial': [
        ('call 0',
         'pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_gather_train pcg_train_dense '
         'pcg_choose_gather_train pcg_train_dense pcg_adam_flush pcg_adam_flush pcg_pick_shuffled_epochs pcg_plan_epochs '
         'pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush pcg_step_scores '
         'pcg_pos_sort'),
    ],
    'n_steps=2/pipelined': [
        ('call 0',
         'pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_train_part pcg_choose_train_part '
         'pcg_dense_select_train pcg_choose_train_part pcg_train_dense pcg_adam_flush pcg_adam_flush '
         'pcg_pick_shuffled_epochs pcg_plan_epochs pcg_choose_train_part pcg_choose_train_part pcg_dense_select_train '
         'pcg_choose_train_part pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
    ],
    'n_steps=2/pipelined_ahead': [
        ('call 0',
         'pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_train_part pcg_choose_train_part '
         'pcg_dense_select_train pcg_choose_train_part pcg_train_dense pcg_adam_flush pcg_adam_flush '
         'pcg_pick_shuffled_epochs pcg_plan_epochs pcg_choose_train_part pcg_choose_train_part pcg_dense_select_train '
         'pcg_choose_train_part pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
    ],
    'n_epochs=2/serial': [
        ('call 0',
         'pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_gather_train pcg_train_dense '
         'pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train '
         'pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush '
         'pcg_adam_flush pcg_pick_shuffled_epochs pcg_plan_epochs pcg_choose_gather_train pcg_train_dense '
         'pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train '
         'pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush '
         'pcg_step_scores pcg_pos_sort'),
    ],
    'n_epochs=2/pipelined': [
        ('call 0',
         'pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_train_part pcg_choose_train_part '
         'pcg_dense_select_train pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part pcg_dense_select_train '
         'pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part '
         'pcg_train_dense pcg_adam_flush pcg_adam_flush pcg_pick_shuffled_epochs pcg_plan_epochs pcg_choose_train_part '
         'pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part '
         'pcg_dense_select_train pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part pcg_dense_select_train '
         'pcg_choose_train_part pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
    ],
    'n_epochs=2/pipelined_ahead': [
        ('call 0',
         'pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_train_part pcg_step_scores pcg_pos_sort '
         'pcg_clf_step pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_dense_select_ahead '
         'pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part '
         'pcg_dense_select_ahead pcg_choose_train_part pcg_train_dense pcg_adam_flush pcg_adam_flush '
         'pcg_pick_shuffled_epochs pcg_plan_epochs pcg_choose_train_part pcg_step_scores pcg_pos_sort pcg_clf_step '
         'pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part '
         'pcg_dense_select_ahead pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_dense_select_ahead '
         'pcg_choose_train_part pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
    ],
    'prefetch/serial': [
        ('call 0',
         'pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_gather_train pcg_train_dense '
         'pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush pcg_plan_epochs '
         'pcg_adam_flush pcg_pick_shuffled_epochs pcg_plan_epochs pcg_pick_shuffled_epochs pcg_plan_epochs '
         'pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train '
         'pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
        ('call 1',
         'pcg_adam_flush pcg_plan_epochs pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense '
         'pcg_choose_gather_train pcg_train_dense pcg_adam_flush pcg_plan_epochs pcg_adam_flush pcg_pick_shuffled_epochs '
         'pcg_plan_epochs pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense '
         'pcg_choose_gather_train pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
        ('call 2',
         'pcg_adam_flush pcg_plan_epochs pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense '
         'pcg_choose_gather_train pcg_train_dense pcg_adam_flush pcg_plan_epochs pcg_adam_flush pcg_pick_shuffled_epochs '
         'pcg_plan_epochs pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense '
         'pcg_choose_gather_train pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
    ],
    'prefetch/pipelined': [
        ('call 0',
         'pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_train_part pcg_choose_train_part '
         'pcg_dense_select_train pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part pcg_train_dense '
         'pcg_adam_flush pcg_plan_epochs pcg_adam_flush pcg_pick_shuffled_epochs pcg_plan_epochs pcg_pick_shuffled_epochs '
         'pcg_plan_epochs pcg_choose_train_part pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part '
         'pcg_dense_select_train pcg_choose_train_part pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
        ('call 1',
         'pcg_adam_flush pcg_plan_epochs pcg_choose_train_part pcg_choose_train_part pcg_dense_select_train '
         'pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part pcg_train_dense pcg_adam_flush '
         'pcg_plan_epochs pcg_adam_flush pcg_pick_shuffled_epochs pcg_plan_epochs pcg_choose_train_part '
         'pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part '
         'pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
        ('call 2',
         'pcg_adam_flush pcg_plan_epochs pcg_choose_train_part pcg_choose_train_part pcg_dense_select_train '
         'pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part pcg_train_dense pcg_adam_flush '
         'pcg_plan_epochs pcg_adam_flush pcg_pick_shuffled_epochs pcg_plan_epochs pcg_choose_train_part '
         'pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part '
         'pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
    ],
    'prefetch/pipelined_ahead': [
        ('call 0',
         'pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_train_part pcg_step_scores pcg_pos_sort '
         'pcg_clf_step pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_dense_select_ahead '
         'pcg_choose_train_part pcg_train_dense pcg_adam_flush pcg_plan_epochs pcg_adam_flush pcg_pick_shuffled_epochs '
         'pcg_plan_epochs pcg_pick_shuffled_epochs pcg_plan_epochs pcg_choose_train_part pcg_step_scores pcg_pos_sort '
         'pcg_clf_step pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_dense_select_ahead '
         'pcg_choose_train_part pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
        ('call 1',
         'pcg_adam_flush pcg_plan_epochs pcg_choose_train_part pcg_step_scores pcg_pos_sort pcg_clf_step '
         'pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part '
         'pcg_train_dense pcg_adam_flush pcg_plan_epochs pcg_adam_flush pcg_pick_shuffled_epochs pcg_plan_epochs '
         'pcg_choose_train_part pcg_step_scores pcg_pos_sort pcg_clf_step pcg_choose_train_part pcg_dense_select_ahead '
         'pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_train_dense pcg_adam_flush '
         'pcg_step_scores pcg_pos_sort'),
        ('call 2',
         'pcg_adam_flush pcg_plan_epochs pcg_choose_train_part pcg_step_scores pcg_pos_sort pcg_clf_step '
         'pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part '
         'pcg_train_dense pcg_adam_flush pcg_plan_epochs pcg_adam_flush pcg_pick_shuffled_epochs pcg_plan_epochs '
         'pcg_choose_train_part pcg_step_scores pcg_pos_sort pcg_clf_step pcg_choose_train_part pcg_dense_select_ahead '
         'pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_train_dense pcg_adam_flush '
         'pcg_step_scores pcg_pos_sort'),
    ],
    'stream/serial': [
        ('call 0',
         'pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_gather_train pcg_train_dense '
         'pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush pcg_plan_epochs '
         'pcg_adam_flush pcg_pick_shuffled_epochs pcg_plan_epochs pcg_choose_gather_train pcg_train_dense '
         'pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush pcg_step_scores '
         'pcg_pos_sort pcg_pick_shuffled_epochs pcg_plan_epochs'),
        ('call 1',
         'pcg_adam_flush pcg_plan_epochs pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense '
         'pcg_choose_gather_train pcg_train_dense pcg_adam_flush pcg_plan_epochs pcg_adam_flush pcg_choose_gather_train '
         'pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush '
         'pcg_step_scores pcg_pos_sort pcg_pick_shuffled_epochs pcg_plan_epochs'),
        ('call 2',
         'pcg_adam_flush pcg_plan_epochs pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense '
         'pcg_choose_gather_train pcg_train_dense pcg_adam_flush pcg_plan_epochs pcg_adam_flush pcg_choose_gather_train '
         'pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush '
         'pcg_step_scores pcg_pos_sort pcg_pick_shuffled_epochs pcg_plan_epochs'),
    ],
    'stream/pipelined': [
        ('call 0',
         'pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_train_part pcg_choose_train_part '
         'pcg_dense_select_train pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part pcg_train_dense '
         'pcg_adam_flush pcg_plan_epochs pcg_adam_flush pcg_pick_shuffled_epochs pcg_plan_epochs pcg_choose_train_part '
         'pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part '
         'pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort pcg_pick_shuffled_epochs pcg_plan_epochs'),
        ('call 1',
         'pcg_adam_flush pcg_plan_epochs pcg_choose_train_part pcg_choose_train_part pcg_dense_select_train '
         'pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part pcg_train_dense pcg_adam_flush '
         'pcg_plan_epochs pcg_adam_flush pcg_choose_train_part pcg_choose_train_part pcg_dense_select_train '
         'pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part pcg_train_dense pcg_adam_flush '
         'pcg_step_scores pcg_pos_sort pcg_pick_shuffled_epochs pcg_plan_epochs'),
        ('call 2',
         'pcg_adam_flush pcg_plan_epochs pcg_choose_train_part pcg_choose_train_part pcg_dense_select_train '
         'pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part pcg_train_dense pcg_adam_flush '
         'pcg_plan_epochs pcg_adam_flush pcg_choose_train_part pcg_choose_train_part pcg_dense_select_train '
         'pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part pcg_train_dense pcg_adam_flush '
         'pcg_step_scores pcg_pos_sort pcg_pick_shuffled_epochs pcg_plan_epochs'),
    ],
    'stream/pipelined_ahead': [
        ('call 0',
         'pcg_adam_flush pcg_plan_epochs pcg_step_scores pcg_pos_sort pcg_choose_train_part pcg_step_scores pcg_pos_sort '
         'pcg_clf_step pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_dense_select_ahead '
         'pcg_choose_train_part pcg_train_dense pcg_adam_flush pcg_plan_epochs pcg_adam_flush pcg_pick_shuffled_epochs '
         'pcg_plan_epochs pcg_choose_train_part pcg_step_scores pcg_pos_sort pcg_clf_step pcg_choose_train_part '
         'pcg_dense_select_ahead pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_train_dense '
         'pcg_adam_flush pcg_step_scores pcg_pos_sort pcg_pick_shuffled_epochs pcg_plan_epochs'),
        ('call 1',
         'pcg_adam_flush pcg_plan_epochs pcg_choose_train_part pcg_step_scores pcg_pos_sort pcg_clf_step '
         'pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part '
         'pcg_train_dense pcg_adam_flush pcg_plan_epochs pcg_adam_flush pcg_choose_train_part pcg_step_scores pcg_pos_sort '
         'pcg_clf_step pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_dense_select_ahead '
         'pcg_choose_train_part pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort pcg_pick_shuffled_epochs '
         'pcg_plan_epochs'),
        ('call 2',
         'pcg_adam_flush pcg_plan_epochs pcg_choose_train_part pcg_step_scores pcg_pos_sort pcg_clf_step '
         'pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part '
         'pcg_train_dense pcg_adam_flush pcg_plan_epochs pcg_adam_flush pcg_choose_train_part pcg_step_scores pcg_pos_sort '
         'pcg_clf_step pcg_choose_train_part pcg_dense_select_ahead pcg_choose_train_part pcg_dense_select_ahead '
         'pcg_choose_train_part pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort pcg_pick_shuffled_epochs '
         'pcg_plan_epochs'),
    ],
    'first_step=1/serial': [
        ('start_epoch_staged', 'pcg_pick_shuffled_epochs pcg_plan_epochs'),
        ('epoch_step(0, defer)',
         'pcg_adam_flush pcg_step_scores pcg_pos_sort pcg_choose_gather_train pcg_train_dense pcg_adam_flush '
         'pcg_choose_gather_train pcg_train_dense pcg_step_scores pcg_pos_sort'),
        ('epoch_run(first_step=1)',
         'pcg_adam_flush pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush '
         'pcg_adam_flush pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush '
         'pcg_step_scores pcg_pos_sort'),
    ],
    'first_step=1/pipelined': [
        ('start_epoch_staged', 'pcg_pick_shuffled_epochs pcg_plan_epochs'),
        ('epoch_step(0, defer)',
         'pcg_adam_flush pcg_step_scores pcg_pos_sort pcg_choose_gather_train pcg_train_dense pcg_adam_flush '
         'pcg_choose_gather_train pcg_train_dense pcg_step_scores pcg_pos_sort'),
        ('epoch_run(first_step=1)',
         'pcg_adam_flush pcg_choose_train_part pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part '
         'pcg_train_dense pcg_adam_flush pcg_adam_flush pcg_choose_train_part pcg_choose_train_part pcg_dense_select_train '
         'pcg_choose_train_part pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
    ],
    'first_step=1/pipelined_ahead': [
        ('start_epoch_staged', 'pcg_pick_shuffled_epochs pcg_plan_epochs'),
        ('epoch_step(0, defer)',
         'pcg_adam_flush pcg_step_scores pcg_pos_sort pcg_choose_gather_train pcg_train_dense pcg_adam_flush '
         'pcg_choose_gather_train pcg_train_dense pcg_step_scores pcg_pos_sort'),
        ('epoch_run(first_step=1)',
         'pcg_adam_flush pcg_choose_train_part pcg_choose_train_part pcg_dense_select_train pcg_choose_train_part '
         'pcg_train_dense pcg_adam_flush pcg_adam_flush pcg_choose_train_part pcg_choose_train_part pcg_dense_select_train '
         'pcg_choose_train_part pcg_train_dense pcg_adam_flush pcg_step_scores pcg_pos_sort'),
    ],
    'plain/touched': [
        ('call 0',
         'pcg_adam_flush pcg_plan_epochs pcg_mark_touched_planned pcg_step_scores pcg_pos_sort pcg_choose_gather_train '
         'pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush '
         'pcg_adam_flush pcg_pick_shuffled_epochs pcg_plan_epochs pcg_mark_touched_planned pcg_step_scores pcg_pos_sort '
         'pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train '
         'pcg_train_dense pcg_adam_flush'),
        ('call 1', ''),
    ],
    'prefetch/touched': [
        ('call 0',
         'pcg_adam_flush pcg_plan_epochs pcg_mark_touched_planned pcg_step_scores pcg_pos_sort pcg_choose_gather_train '
         'pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush '
         'pcg_plan_epochs pcg_mark_touched_planned pcg_adam_flush pcg_pick_shuffled_epochs pcg_plan_epochs '
         'pcg_mark_touched_planned pcg_pick_shuffled_epochs pcg_plan_epochs pcg_mark_touched_planned pcg_step_scores '
         'pcg_pos_sort pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense '
         'pcg_choose_gather_train pcg_train_dense pcg_adam_flush'),
        ('call 1',
         'pcg_adam_flush pcg_plan_epochs pcg_mark_touched_planned pcg_step_scores pcg_pos_sort pcg_choose_gather_train '
         'pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush '
         'pcg_plan_epochs pcg_mark_touched_planned pcg_adam_flush pcg_pick_shuffled_epochs pcg_plan_epochs '
         'pcg_mark_touched_planned pcg_step_scores pcg_pos_sort pcg_choose_gather_train pcg_train_dense '
         'pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush'),
        ('call 2',
         'pcg_adam_flush pcg_plan_epochs pcg_mark_touched_planned pcg_step_scores pcg_pos_sort pcg_choose_gather_train '
         'pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush '
         'pcg_plan_epochs pcg_mark_touched_planned pcg_adam_flush pcg_pick_shuffled_epochs pcg_plan_epochs '
         'pcg_mark_touched_planned pcg_step_scores pcg_pos_sort pcg_choose_gather_train pcg_train_dense '
         'pcg_choose_gather_train pcg_train_dense pcg_choose_gather_train pcg_train_dense pcg_adam_flush'),
    ],
}
