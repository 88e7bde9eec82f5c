"""How the training step of ONE configuration (batch shapes + step options: Trainer._graph_key) is issued: eager
launches, a replayed HIP graph, or a launch plan (csrc/plan.hip).  StepPolicy holds every bit of decision state of that
configuration; the Trainer asks `next_action()`, does what it says on the device and reports what happened.  Nothing here
touches the device (no torch, no library): the whole table is tested on the CPU (tests/test_step_policy.py).

    phase                          rule
    -----------------------------  -------------------------------------------------------------------------------------
    warm-up                        WARM eager steps: 2 if a capture follows whatever the timing says, else 4
    last warm-up step, auto        timed: host_bound = host_ms > HOST_BOUND x dev_ms, eager_ms = dev_ms; capture next when
                                   the plan is on or the host is the limit, else eager verdict
    last warm-up step, forced      plain eager step, capture next; no eager_ms: never a replay check, never a watch
    capture succeeded              the same step replays it
    plan refused                   the plan is off for the key for good; a HIP graph is tried in the same step iff one is
                                   allowed and (forced mode or host_bound), else eager verdict
    capture raised                 swallowed (eager verdict, plan off for the key) iff the capture was the watch's idea
                                   or a PLAN capture in auto; otherwise the error is the caller's
    second replay, auto            timed once (when eager_ms is known): the capture is dropped for an unwatched eager
                                   verdict when it took more than PLAN_SLACK / GRAPH_SLACK x eager_ms
    watched eager verdict fires    verdict withdrawn, eager_ms = the watch's recent period, replay check re-armed, capture
                                   next (plan if still on for the key, else HIP graph); nothing is watched a second time

Watch rule: an eager verdict is watched iff eager_ms is known, the verdict has not been withdrawn before and a capture
kind is still permitted for the key.  `graph_allowed` = False (a gradient reducer whose collectives may not be captured
into a HIP graph) therefore never yields CAPTURE_GRAPH, in any state; a key for which neither kind is permitted is under
an eager verdict from its first step."""

EAGER, EAGER_TIMED, EAGER_WATCHED = 'eager', 'eager_timed', 'eager_watched'
CAPTURE_PLAN, CAPTURE_GRAPH = 'capture_plan', 'capture_graph'
REPLAY, REPLAY_TIMED = 'replay', 'replay_timed'

# eager warm-up steps before the capture: 4 when the host-vs-device timing of the last one decides between eager launches
# and a HIP graph (the first steps still grow workspaces and the allocator's pools); 2 when a capture follows whatever the
# timing says - the step then runs as a plan from the THIRD step on, so that a benchmark's warm-up of >= 3 steps leaves
# only replays in its timed region
WARM_TIMING_DECIDES, WARM_CAPTURE_FOLLOWS = 4, 2
# last warm-up step, mode 'auto': is the eager step bound by the host (launch time ~ device time) or by the device?  A
# replayed graph removes the host cost but measured 5 % SLOWER than the eager two-stream schedule when the device is the
# limit (ResNet-50 b=256: 22.1 vs 21.0 ms), and 1.55x faster when the host is (b=8: 5.5 vs 8.6 ms) - profiles/README.md.
HOST_BOUND = 0.75
# the prediction is checked once: a nearly host-bound eager step can still beat the replay (ResNet-50 b=128: 12.2 ms eager
# vs 13.3 ms replayed), so the second replay is timed and a HIP graph dropped if it is not faster than the eager step it
# was meant to replace
GRAPH_SLACK = 0.98
# (a plan is the eager schedule minus the host - the same launches on the same streams: it cannot be slower by
# construction, and this ONE sample also sees whatever else is on the device at that moment, e.g. the loader's
# host-to-device copy of the next batch (a plan was dropped that way in a --host-inputs run).  It is given up only when it
# measures grossly slower; what it buys - independence from the host's load - no quiet-box comparison can show)
PLAN_SLACK = 1.25


class StepPolicy(object):
    """mode: 'auto' (capture when it pays) or anything else (forced: flag graph = 1); plan: launch plans are on;
    graph_allowed: this trainer's step may be captured into a plain HIP graph (no reducer, or flag graph_dp)."""

    __slots__ = ('auto', 'graph_allowed', 'warm', 'n', 'plan', 'host_bound', 'eager_ms', 'eager', 'watched', 'withdrawn',
                 'captured', 'replays', 'graph_ms')

    def __init__(self, mode, plan, graph_allowed):
        self.auto = mode == 'auto'
        self.graph_allowed = bool(graph_allowed)
        self.warm = WARM_CAPTURE_FOLLOWS if (not self.auto or plan) else WARM_TIMING_DECIDES
        self.n = 0                   # eager warm-up steps done
        self.plan = bool(plan)       # launch plans are (still) on for this key
        self.host_bound = False      # the timed warm-up step was limited by the host
        self.eager_ms = None         # device time of the eager step the replay is checked against (auto only)
        self.eager = not (plan or graph_allowed)     # eager verdict in force (from the start: nothing may be captured)
        self.watched = False         # ... and re-examined while it is (trainer.EagerWatch)
        self.withdrawn = False       # the watch withdrew a verdict of this key once
        self.captured = None         # 'plan' / 'graph': the kind of the live capture
        self.replays = 0             # replays since the check was (re-)armed
        self.graph_ms = None         # the timed second replay: the check is done

    @classmethod
    def eager_verdict(cls, eager_ms, mode='auto', plan=True, graph_allowed=True):
        """The state of a configuration found device-bound on its last warm-up step: eager verdict based on `eager_ms`,
        watched where the watch rule allows it."""
        p = cls(mode, plan, graph_allowed)
        p.n, p.eager_ms = p.warm, float(eager_ms)
        p._settle_eager()
        return p

    # -- the one question ----------------------------------------------------------------------------------------
    def next_action(self):
        if self.eager:
            return EAGER_WATCHED if self.watched else EAGER
        if self.captured is not None:
            return REPLAY_TIMED if self._check_armed() and self.replays == 1 else REPLAY
        if self.n < self.warm:
            return EAGER_TIMED if (self.auto and self.n == self.warm - 1) else EAGER
        return CAPTURE_PLAN if self.plan else CAPTURE_GRAPH

    # -- what happened -------------------------------------------------------------------------------------------
    def eager_done(self):
        """A plain eager step ran (only warm-up steps count)."""
        self.n = min(self.n + 1, self.warm)

    def eager_timed(self, host_ms, dev_ms):
        """The last warm-up step of mode 'auto', timed on the host (launches) and on the device."""
        self.n = self.warm
        self.host_bound = host_ms > HOST_BOUND * dev_ms
        self.eager_ms = dev_ms
        if not (self.plan or self.host_bound):
            self._settle_eager()

    def captured_as(self, kind):
        self.captured = kind

    def plan_refused(self):
        """The recorded step holds something a plan cannot re-issue: the HIP graph (when one is allowed and either asked
        for or worth it: the host is the limit) or eager launches serve it."""
        self.plan = False
        if not (self.graph_allowed and (not self.auto or self.host_bound)):
            self._settle_eager()

    def capture_failed(self):
        """A capture raised.  False: the error is the caller's to raise (the state is left as it was).
        A capture needs its own pool for the step's tensors, next to the blocks the eager steps keep cached.  When the
        capture was the WATCH's idea (a verdict withdrawn after many eager steps) and it does not fit, the configuration
        simply stays eager; a capture the configuration started with fails as it always did.  The same holds for a
        launch-plan recording in mode 'auto': the plan is an optimisation of a step that already ran eagerly twice -
        whatever made its capture fail (memory, a runtime that refuses the capture with the communicators of a multi-rank
        job alive, ...) must not take the job down.  A forced capture asked for one and still gets the error."""
        if not (self.withdrawn or (self.plan and self.auto)):
            return False
        self.plan = False
        self._settle_eager()
        return True

    def replay_done(self):
        if self._check_armed():
            self.replays += 1

    def replay_timed(self, ms):
        """The second replay took `ms` on the device.  False: the capture is dropped, eager launches from now on."""
        self.replays += 1
        self.graph_ms = ms
        if ms > (PLAN_SLACK if self.captured == 'plan' else GRAPH_SLACK) * self.eager_ms:
            self.captured, self.eager, self.watched = None, True, False
            return False
        return True

    def watch_fired(self, recent_ms):
        """The eager step has been running slower than a replay would for a window of steps: the host has become the limit
        after the verdict was taken.  The next step captures; the check of the second replay against the eager time - now
        the recent one, loader wait excluded - applies again."""
        self.eager, self.watched, self.withdrawn = False, False, True
        self.eager_ms, self.replays, self.graph_ms = recent_ms, 0, None

    # ------------------------------------------------------------------------------------------------------------
    def _check_armed(self):
        return self.auto and self.graph_ms is None and self.eager_ms is not None

    def _settle_eager(self):
        """Eager verdict; THE watch rule."""
        self.eager, self.captured = True, None
        self.watched = self.eager_ms is not None and not self.withdrawn and (self.plan or self.graph_allowed)
