"""The hand-overs of one training step between its engine (immtsf.train: GraphedStep, PhasedStep, FlagStep) and the ops (immtsf.ops).

An engine installs one StepPlan per step it runs or captures and switches what the plan offers between the step's phases; an op asks
`current()` through the named operations below and never sees the flag words.  Outside an engine `current()` offers nothing.  One
process-wide slot, not a thread-local: the backward of a GPU graph runs on autograd's device worker thread."""
import contextlib
import gc

import torch

from . import _lib


def collect_before_capture():
    """Called in front of every capture of the project's own (the step engines, the seam graph, EvalStep).  On ROCm the destructor of a
    torch.cuda.CUDAGraph synchronises the device, which is illegal while a stream captures: a dead engine that still sits in a reference
    cycle (FlagStep <-> FlatTrainer._flush_cb) and is collected INSIDE the next engine's capture throws from that destructor and the
    process aborts -- whenever the collector's counters happen to trip there.  torch.cuda.graph() collected on entry by itself up to
    torch 2.8; this is that collection, for these captures only."""
    gc.collect()


class StepPlan:
    # what an engine switches between the phases of a step, with offering()
    OFFERS = ("fold_stream", "fold_flag", "gate", "head_flag", "hold_params", "wgrad_flags", "defer", "tail_flag", "ttf_flag", "announce")

    def __init__(self, err=None, timeout_ms=50):
        self.err, self.timeout_ms = err, timeout_ms     # the flag waits below: time-out report address (FlagStep's guard word), time-out
        # the text side's forward: MMF_XAttn_Add's fold (parameters only) on `fold_stream`, handed over by `fold_flag` or a stream wait
        self.fold_stream = self.fold_flag = None
        # scheduling gate, (flag, time-out report address): TTF_T2V_XAttn's backward sets it behind its row-bound kernels, the patch
        # encoder's backward (parameter gradients only, on the backbone's stream) spins on it first -- when a forward armed it
        self.gate = self._armed = None
        self.head_flag = self.head_dy_ptr = None        # "dY_ts is ready": a head whose kernel publishes it takes it
        self.hold_params, self._params = False, []      # PhasedStep: the head's parameter-gradient work waits for run_params()
        # the backbone's backward: weight gradients leave for the parameter branch as `jobs_b`, each behind a flag of the pool
        self.wgrad_flags, self.jobs_b = [], []
        # the text side's backward: the last `defer` launches of MMF_XAttn_Add's parameter chain (behind `tail_flag`) and TTF_T2V_XAttn's
        # early weight gradients (behind `ttf_flag`) leave for the parameter branch as `jobs`
        self.defer, self.tail_flag, self.ttf_flag, self.tail_set, self.jobs = 0, None, None, False, []
        self.announce = None            # FlagStep, data parallel: FlatTrainer's bucket hooks announce the bucket through this instead

    @contextlib.contextmanager
    def offering(self, **fields):
        """the named offers hold for the body; on the way out, raised or not, the previous values are back"""
        if not set(fields) <= set(self.OFFERS):
            raise AttributeError(f"StepPlan has no offer {sorted(set(fields) - set(self.OFFERS))[0]!r}")
        before = {k: getattr(self, k) for k in fields}
        self.__dict__.update(fields)
        try:
            yield self
        finally:
            self.__dict__.update(before)

    def set(self, flag, stream):
        """`stream` (raw handle) sets the device flag at address `flag`"""
        _lib.check(_lib.load().immtsf_flag_set(flag, stream), "flag_set")

    def wait(self, flag, stream, err=None):
        """`stream` spins on `flag`; after `timeout_ms` it gives up and reports to `err` (default: the plan's)"""
        _lib.check(_lib.load().immtsf_flag_wait(flag, self.err if err is None else err, self.timeout_ms, stream), "flag_wait")

    def fold(self, launch, *uses):
        """run `launch(raw stream)` on the fold stream, hand its result (and `uses`) to the current stream; False: none offered"""
        L = self.fold_stream
        if L is None:
            return False
        cur = torch.cuda.current_stream()
        for t in uses:
            t.record_stream(L)
        launch(L.cuda_stream)
        if self.fold_flag is not None:
            self.set(self.fold_flag, L.cuda_stream)
            self.wait(self.fold_flag, cur.cuda_stream)
        else:
            cur.wait_stream(L)
        return True

    def arm_gate(self):
        """a forward whose backward will set the gate: -> the gate's flag address (None: no gate offered)"""
        if self.gate is not None:
            self._armed = torch.cuda.current_stream().cuda_stream
            return self.gate[0]

    def wait_gate(self):
        """the current stream spins on the gate when a forward on ANOTHER stream armed it (a hint: it gives up after `timeout_ms`)"""
        if self.gate is not None and self._armed not in (None, torch.cuda.current_stream().cuda_stream):
            self.wait(self.gate[0], _lib.stream_ptr(), err=self.gate[1])

    def take_head_flag(self, dY):
        """-> the head flag, handed out once (None: not offered); `dY`: the buffer the kernel publishes"""
        flag, self.head_flag = self.head_flag, None
        if flag is not None:
            self.head_dy_ptr = dY.data_ptr()
        return flag

    def defer_params(self, fn):
        self._params.append(fn)

    def run_params(self):
        work, self._params = self._params, []
        for fn in work:
            fn()

    @property
    def wgrad_open(self):
        return bool(self.wgrad_flags)

    def defer_wgrad(self, launch, keep=(), ttf=False):
        """a weight gradient `launch(raw stream)` leaves the current stream: a flag (the pool's next, or `ttf`: the TTF phase flag) is
        set here, and a job waits for it on the parameter branch, then launches.  `keep`: what the launch reads, held until then."""
        flag, jobs = (self.ttf_flag, self.jobs) if ttf else (self.wgrad_flags.pop(), self.jobs_b)
        self.set(flag, _lib.stream_ptr())

        def job(stream, keep=keep):
            self.wait(flag, stream)
            launch(stream)
        jobs.append(job)

    def set_tail(self):
        self.set(self.tail_flag, _lib.stream_ptr())
        self.tail_set = True            # (the parameter branch waits for the TAIL flag only when somebody set it)


_active = None
_IDLE = StepPlan()


def current() -> StepPlan:
    return _IDLE if _active is None else _active


@contextlib.contextmanager
def install(plan: StepPlan):
    """`plan` is current() for the body; on the way out, raised or not, it is uninstalled and the work it still holds dropped"""
    global _active
    if _active is not None:
        raise RuntimeError("a step plan is already installed: one step at a time")
    _active = plan
    try:
        yield plan
    finally:
        _active = None
        plan._params, plan.jobs, plan.jobs_b = [], [], []
