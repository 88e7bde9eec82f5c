"""How a training step is issued (eager launches, HIP graph, launch plan): the decision table of
convnet.pytorch_amd/step_policy.py, and Trainer._graph_step driving it.  CPU tests: the policy touches no device, and the
driver runs on the emulator with the device-facing methods (_capture / _feed / _replay / _timed) replaced by fakes whose
'replay' runs the real step body."""
import ast
import itertools
import os

import pytest
import torch

from helpers import ROOT

import convnet_amd as ca

SP = ca.step_policy
P = SP.StepPolicy
ALL = list(itertools.product(('auto', '1'), (True, False), (True, False)))       # mode x plan x graph_allowed


def drive(p, n):
    """n plain steps of a policy that needs nothing but eager steps reported: the actions it asked for."""
    acts = []
    for _ in range(n):
        a = p.next_action()
        acts.append(a)
        assert a in (SP.EAGER, SP.EAGER_WATCHED), a
        p.eager_done()
    return acts


def warmed(mode, plan, ga, host_ms=1.0, dev_ms=100.0):
    """A policy behind its warm-up (auto: the last step timed host_ms / dev_ms) + the actions of the warm-up."""
    p, acts = P(mode, plan, ga), []
    while p.n < p.warm:
        acts.append(p.next_action())
        if acts[-1] is SP.EAGER_TIMED:
            p.eager_timed(host_ms, dev_ms)
        else:
            p.eager_done()
    return p, acts


def test_the_policy_module_is_pure():
    """No torch, no library, no sibling module: what it decides can be tested anywhere."""
    tree = ast.parse(open(os.path.join(ROOT, 'convnet.pytorch_amd', 'step_policy.py')).read())
    imports = [n for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert imports == []
    assert (SP.WARM_CAPTURE_FOLLOWS, SP.WARM_TIMING_DECIDES, SP.HOST_BOUND, SP.PLAN_SLACK, SP.GRAPH_SLACK) == \
        (2, 4, 0.75, 1.25, 0.98)
    w = ca.trainer.EagerWatch(1.0)
    assert (w.window, w.factor) == (9, 1.2)


@pytest.mark.parametrize('mode,plan,ga', ALL)
def test_warm_up_lengths_and_what_follows(mode, plan, ga):
    if not (plan or ga):                    # nothing may be captured: eager from the start, nothing to time or watch for
        assert drive(P(mode, plan, ga), 30) == [SP.EAGER] * 30
        return
    p, acts = warmed(mode, plan, ga, host_ms=90.0, dev_ms=100.0)          # (auto: host-bound)
    if mode == '1':
        assert acts == [SP.EAGER, SP.EAGER]                               # never timed: no eager_ms, no check, no watch
        assert p.eager_ms is None
    elif plan:
        assert acts == [SP.EAGER, SP.EAGER_TIMED]
    else:
        assert acts == [SP.EAGER] * 3 + [SP.EAGER_TIMED]
    if plan:
        assert p.next_action() is SP.CAPTURE_PLAN
    else:
        assert p.next_action() is SP.CAPTURE_GRAPH


@pytest.mark.parametrize('plan,ga', [(True, True), (True, False), (False, True)])
def test_host_bound_boundary_of_the_timed_step(plan, ga):
    below, _ = warmed('auto', plan, ga, host_ms=75.0, dev_ms=100.0)       # host_ms > 0.75 x dev_ms, strictly
    above, _ = warmed('auto', plan, ga, host_ms=75.01, dev_ms=100.0)
    assert (below.host_bound, above.host_bound) == (False, True)
    assert below.eager_ms == above.eager_ms == 100.0
    if plan:                                # a plan follows whatever the timing says
        assert below.next_action() is above.next_action() is SP.CAPTURE_PLAN
    else:
        # device-bound: eager verdict, watched against the timed step where a capture could still follow
        assert drive(below, 5) == [SP.EAGER_WATCHED] * 5
        assert above.next_action() is SP.CAPTURE_GRAPH


@pytest.mark.parametrize('mode,ga,host_bound', itertools.product(('auto', '1'), (True, False), (True, False)))
def test_plan_refused(mode, ga, host_bound):
    p, _ = warmed(mode, True, ga, host_ms=90.0 if host_bound else 10.0, dev_ms=100.0)
    assert p.next_action() is SP.CAPTURE_PLAN
    p.plan_refused()
    assert p.plan is False
    if ga and (mode == '1' or host_bound):          # (mode '1': the review's KeyError('use') case)
        assert p.next_action() is SP.CAPTURE_GRAPH
        p.captured_as('graph')
        assert p.next_action() is SP.REPLAY
        return
    # eager verdict; watched iff the timed step gave a reference AND a HIP graph could still follow
    want = SP.EAGER_WATCHED if (mode == 'auto' and ga) else SP.EAGER
    assert drive(p, 20) == [want] * 20
    if want is SP.EAGER_WATCHED:
        p.watch_fired(150.0)
        assert p.next_action() is SP.CAPTURE_GRAPH      # the plan is off for this key for good


def test_capture_failure_swallowed_or_raised():
    """Swallowed iff the capture was the watch's idea (withdrawn verdict) or a PLAN capture in auto."""
    # not withdrawn, plan capture in auto: swallowed; watched iff a HIP graph may still follow
    for ga in (True, False):
        p, _ = warmed('auto', True, ga)
        assert p.next_action() is SP.CAPTURE_PLAN and p.capture_failed() is True
        assert p.plan is False and drive(p, 12) == [SP.EAGER_WATCHED if ga else SP.EAGER] * 12
    # not withdrawn, not a plan capture in auto: the caller's error, nothing changes
    for p, want in ((warmed('1', True, True)[0], SP.CAPTURE_PLAN), (warmed('1', False, True)[0], SP.CAPTURE_GRAPH),
                    (warmed('auto', False, True, host_ms=90.0)[0], SP.CAPTURE_GRAPH)):
        assert p.next_action() is want and p.capture_failed() is False and p.next_action() is want
    p, _ = warmed('auto', True, True, host_ms=90.0)         # ... the HIP graph that follows a refusal included
    p.plan_refused()
    assert p.next_action() is SP.CAPTURE_GRAPH and p.capture_failed() is False and p.next_action() is SP.CAPTURE_GRAPH
    # withdrawn, plan capture / HIP-graph capture: swallowed, eager and UNWATCHED from then on
    for plan in (True, False):
        p = P.eager_verdict(100.0, mode='auto', plan=plan, graph_allowed=True)
        assert drive(p, 3) == [SP.EAGER_WATCHED] * 3
        p.watch_fired(130.0)
        assert p.next_action() is (SP.CAPTURE_PLAN if plan else SP.CAPTURE_GRAPH)
        assert p.capture_failed() is True
        assert drive(p, 30) == [SP.EAGER] * 30
    # a failed plan capture, watched, withdrawn, and the HIP graph tried then fails too: swallowed as well
    p, _ = warmed('auto', True, True, host_ms=90.0)
    assert p.capture_failed() is True and p.next_action() is SP.EAGER_WATCHED
    p.watch_fired(130.0)
    assert p.next_action() is SP.CAPTURE_GRAPH and p.capture_failed() is True and drive(p, 9) == [SP.EAGER] * 9


@pytest.mark.parametrize('kind,ms,keep', [('plan', 124.99, True), ('plan', 125.0, True), ('plan', 125.01, False),
                                          ('graph', 97.99, True), ('graph', 98.0, True), ('graph', 98.01, False)])
def test_second_replay_is_checked_against_the_eager_step(kind, ms, keep):
    p, _ = warmed('auto', kind == 'plan', True, host_ms=90.0, dev_ms=100.0)
    assert p.next_action() is (SP.CAPTURE_PLAN if kind == 'plan' else SP.CAPTURE_GRAPH)
    p.captured_as(kind)
    assert p.next_action() is SP.REPLAY                   # the capturing step replays
    p.replay_done()
    assert p.next_action() is SP.REPLAY_TIMED             # the second replay is timed, once
    assert p.replay_timed(ms) is keep
    if keep:
        for _ in range(20):
            assert p.next_action() is SP.REPLAY
            p.replay_done()
    else:
        assert drive(p, 20) == [SP.EAGER] * 20            # dropped: eager and unwatched


@pytest.mark.parametrize('plan', (True, False))
def test_forced_mode_never_times_a_replay(plan):
    p, _ = warmed('1', plan, True)
    p.captured_as('plan' if plan else 'graph')
    for _ in range(10):
        assert p.next_action() is SP.REPLAY
        p.replay_done()


@pytest.mark.parametrize('plan,ms,keep', [(True, 37.4, True), (True, 37.6, False), (False, 29.3, True), (False, 29.5, False)])
def test_withdrawal_rearms_the_replay_check_against_the_recent_period(plan, ms, keep):
    p = P.eager_verdict(20.0, mode='auto', plan=plan, graph_allowed=True)
    assert p.n == p.warm and drive(p, 13) == [SP.EAGER_WATCHED] * 13
    p.watch_fired(30.0)
    assert p.withdrawn and p.eager_ms == 30.0
    kind = 'plan' if plan else 'graph'
    assert p.next_action() is (SP.CAPTURE_PLAN if plan else SP.CAPTURE_GRAPH)
    p.captured_as(kind)
    assert p.next_action() is SP.REPLAY
    p.replay_done()
    assert p.next_action() is SP.REPLAY_TIMED
    assert p.replay_timed(ms) is keep                     # 1.25 x 30 = 37.5, 0.98 x 30 = 29.4
    assert p.next_action() is (SP.REPLAY if keep else SP.EAGER)


def _successors(p):
    """Every event the driver may report for the action the policy asked for -> copies of the policy after it."""
    def after(fn):
        q = P.__new__(P)
        for s in P.__slots__:
            setattr(q, s, getattr(p, s))
        fn(q)
        return q
    a = p.next_action()
    if a is SP.EAGER:
        return a, [after(lambda q: q.eager_done())]
    if a is SP.EAGER_TIMED:
        return a, [after(lambda q: q.eager_timed(10.0, 100.0)), after(lambda q: q.eager_timed(90.0, 100.0))]
    if a is SP.EAGER_WATCHED:
        return a, [after(lambda q: q.eager_done()), after(lambda q: q.watch_fired(2.0 * q.eager_ms))]
    if a in (SP.CAPTURE_PLAN, SP.CAPTURE_GRAPH):
        kind = 'plan' if a is SP.CAPTURE_PLAN else 'graph'
        out = [after(lambda q: q.captured_as(kind)), after(lambda q: q.capture_failed())]
        if a is SP.CAPTURE_PLAN:
            out.append(after(lambda q: q.plan_refused()))
        return a, out
    if a is SP.REPLAY:
        return a, [after(lambda q: q.replay_done())]
    assert a is SP.REPLAY_TIMED
    return a, [after(lambda q: q.replay_timed(0.5 * q.eager_ms)), after(lambda q: q.replay_timed(2.0 * q.eager_ms))]


@pytest.mark.parametrize('mode,plan', itertools.product(('auto', '1'), (True, False)))
def test_no_hip_graph_is_ever_captured_where_none_is_allowed(mode, plan):
    """A reducer whose collectives may not be captured (graph_allowed = False): over EVERY sequence of events up to 24
    steps - warm-up 4, capture, check 2, verdict, watch, withdrawal and the same again fit twice - no state asks for
    CAPTURE_GRAPH.  (States are compared by value, so the search closes long before the bound.)"""
    state = lambda q: tuple(getattr(q, s) for s in P.__slots__)
    frontier, seen, actions = [P(mode, plan, False)], set(), set()
    for depth in range(24):
        nxt = []
        for p in frontier:
            a, succ = _successors(p)
            actions.add(a)
            for q in succ:
                if state(q) not in seen:
                    seen.add(state(q))
                    nxt.append(q)
        frontier = nxt
    assert not frontier, 'the search did not close'
    assert SP.CAPTURE_GRAPH not in actions
    assert (SP.CAPTURE_PLAN in actions) == plan
    # (the same search with a HIP graph allowed does find it: the property is not vacuous)
    frontier, seen2, actions2 = [P(mode, plan, True)], set(), set()
    for depth in range(24):
        nxt = []
        for p in frontier:
            a, succ = _successors(p)
            actions2.add(a)
            nxt += [q for q in succ if state(q) not in seen2 and not seen2.add(state(q))]
        frontier = nxt
    assert SP.CAPTURE_GRAPH in actions2


# ---- the driver: Trainer._graph_step on the emulator -------------------------------------------------------------------
# (one basic block per stage, stride-2 projections included: an emulated step of it takes seconds, not tens of seconds)
KW = dict(block='basic', layers=[1, 1, 1, 1], expansion=1, width=(8, 8, 8, 8), inplanes=8, num_classes=16)


def batches(sizes, seed=9):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(b, 3, 32, 32, generator=g), torch.randint(0, 16, (b,), generator=g)) for b in sizes]


class StubReducer(object):
    """What Trainer._body asks of a gradient reducer, on one rank: nothing to reduce."""
    comm, enabled = object(), True

    def reset(self):
        pass

    def finish(self):
        pass


class Fakes(object):
    """The device-facing methods of a Trainer replaced: a 'capture' is a record, its 'replay' runs the real step body."""

    def __init__(self, tr, refuse=(), fail=False, host_ms=90.0, dev_ms=100.0, replay_ms=50.0):
        self.tr, self.refuse, self.fail = tr, refuse, fail
        self.host_ms, self.dev_ms, self.replay_ms, self.replayed = host_ms, dev_ms, replay_ms, False
        self.captures = []            # (batch size, plan) of every capture attempted
        tr._graph_ok = lambda inputs, target: True
        tr._capture, tr._feed, tr._replay, tr._timed = self.capture, self.feed, self.replay, self.timed

    def capture(self, inputs, target, chunk_batch, key, plan=False):
        self.captures.append((inputs.shape[0], plan))
        if plan and (self.refuse is True or inputs.shape[0] in self.refuse):
            raise ca.trainer.PlanRefused('injected: a node no plan can re-issue')
        if self.fail:
            raise RuntimeError('injected: the capture does not fit')
        return {'key': key, 'plan': object() if plan else None, 'chunk': chunk_batch}

    def feed(self, st, inputs, target):
        st['batch'] = (inputs, target)

    def replay(self, st):
        self.replayed = True
        steps = self.tr.training_steps           # (_graph_step advances it itself)
        st['out'], st['loss'], st['grad'] = self.tr._body(st['batch'][0], st['batch'][1], True, st['chunk'])
        self.tr.training_steps = steps

    def timed(self, fn):
        self.replayed = False
        res = fn()
        return res, self.host_ms, (self.replay_ms if self.replayed else self.dev_ms)


def make_trainer(mode, reducer=False):
    import sys
    torch.manual_seed(123)
    model = sys.modules['convnet_amd.models.resnet'].ResNetImagenet(**KW)
    tr = ca.Trainer(model, ca.CrossEntropyLoss(), ca.OptimRegime(model, model.regime), device='cpu', dtype=torch.float32,
                    print_freq=10 ** 9)
    tr._graph_mode, tr._use_graph, tr._plan = mode, mode != '0', True
    if reducer:
        tr.reducer = StubReducer()
    return tr


def losses(tr, data):
    return [tr.train([b])['loss'] for b in data]


@pytest.fixture
def watch_on_cpu(monkeypatch):
    """A watched eager step marks the device timeline: no device here, the watch never fires unless told to."""
    fire = {'at': None, 'n': 0}

    def step(self, stream, wait_ms=0.0):
        fire['n'] += 1
        return fire['n'] == fire['at']
    monkeypatch.setattr(ca.trainer.EagerWatch, 'step', step)
    monkeypatch.setattr(ca.trainer.EagerWatch, 'recent_ms', lambda self: 130.0)
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda device=None: None)
    return fire


@pytest.fixture(scope='module')
def eager_losses():
    return losses(make_trainer('0'), batches([2] * 7))


def test_fake_plan_reproduces_the_eager_step(eager_losses):
    tr = make_trainer('1')
    f = Fakes(tr)
    assert losses(tr, batches([2] * 5)) == eager_losses[:5]
    assert f.captures == [(2, True)] and tr.training_steps == 5
    (rec,) = tr._gstates.values()
    assert rec['graph'].get('plan') is not None and rec['policy'].captured == 'plan'


@pytest.mark.parametrize('mode,reducer,host_ms,plain_graph', [
    ('1', False, 90.0, True),            # forced: the HIP graph serves it (used to die with KeyError('use'))
    ('1', True, 90.0, False),            # ... but never with a reducer's collectives inside
    ('auto', False, 90.0, True),         # host-bound: HIP graph
    ('auto', True, 90.0, False),
    ('auto', False, 10.0, False),        # device-bound: eager launches, watched
    ('auto', True, 10.0, False),         # ... unwatched with a reducer: no later HIP-graph capture either
])
def test_a_refused_plan_leaves_the_job_running(mode, reducer, host_ms, plain_graph, eager_losses, watch_on_cpu):
    tr = make_trainer(mode, reducer)
    f = Fakes(tr, refuse=True, host_ms=host_ms)
    watch_on_cpu['at'] = 2               # a watch, where one is armed, fires on its second step
    n = 7 if (mode == 'auto' and not reducer and not plain_graph) else 5
    assert losses(tr, batches([2] * n)) == eager_losses[:n]
    (rec,) = tr._gstates.values()
    pol = rec['policy']
    if plain_graph:
        assert f.captures == [(2, True), (2, False)]
        assert rec['graph'] is not None and rec['graph'].get('plan') is None and pol.captured == 'graph'
    elif mode == 'auto' and not reducer:
        # the watch fired: the HIP graph is captured after all (the plan stays off), and kept
        assert f.captures == [(2, True), (2, False)] and pol.withdrawn and pol.captured == 'graph'
        assert rec['watch'] is None
    else:
        assert f.captures == [(2, True)]
        assert rec['graph'] is None and pol.eager and not pol.watched and rec['watch'] is None


def test_a_failed_capture_in_auto_stays_eager_and_in_forced_mode_raises(eager_losses, watch_on_cpu):
    tr = make_trainer('auto')
    f = Fakes(tr, fail=True, host_ms=10.0)
    watch_on_cpu['at'] = 3
    assert losses(tr, batches([2] * 7)) == eager_losses
    (rec,) = tr._gstates.values()
    # the plan capture failed: eager, watched; the watch fired, the HIP-graph capture failed too: eager for good
    assert f.captures == [(2, True), (2, False)]
    assert rec['graph'] is None and rec['policy'].eager and not rec['policy'].watched and rec['policy'].withdrawn
    tr = make_trainer('1')
    f = Fakes(tr, fail=True)
    data = batches([2] * 3)
    losses(tr, data[:2])
    with pytest.raises(RuntimeError, match='injected'):
        tr.train([data[2]])


def test_at_most_four_keys_hold_a_capture_and_an_eager_verdict_outlives_them(watch_on_cpu):
    tr = make_trainer('auto')

    def body(inputs, target, training, chunk_batch):       # (bookkeeping only: any step body will do)
        tr.training_steps += 1
        return torch.zeros(inputs.shape[0], 16), torch.zeros(()), None
    tr._body = body
    f = Fakes(tr, refuse=(9,), host_ms=10.0)        # device-bound; the plan of batch size 9 is refused: eager, watched
    (z,) = batches([9])
    hot = batches([4])[0]
    for _ in range(3):
        tr.train([z])
    (zkey,) = tr._gstates.keys()
    assert tr._gstates[zkey]['policy'].eager and tr._gstates[zkey]['policy'].watched
    for _ in range(4):
        tr.train([hot])
    hot_capture = [r['graph'] for r in tr._gstates.values() if r['graph'] is not None]
    assert len(hot_capture) == 1
    for b in (2, 3, 5, 6, 7):                       # five more configurations, the hot one used in between
        for x in batches([b] * 4):
            tr.train([x])
            assert sum(r['graph'] is not None for r in tr._gstates.values()) <= 4
            assert sum(not r['policy'].eager for r in tr._gstates.values()) <= 4
        tr.train([hot])
        tr.train([z])
    live = [r['graph'] for r in tr._gstates.values() if r['graph'] is not None]
    assert len(live) == 4 and any(g is hot_capture[0] for g in live)       # least recently USED out: never the hot one
    assert f.captures.count((4, True)) == 1 and f.captures.count((9, True)) == 1 and (9, False) not in f.captures
    assert tr._gstates[zkey]['policy'].eager and tr._gstates[zkey]['watch'] is not None
    assert not any(k[0][0] in (2, 3) for k in tr._gstates)                  # (the two oldest are the ones that went)
