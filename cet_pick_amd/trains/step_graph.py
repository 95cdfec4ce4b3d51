"""The captured-step driver both step engines derive from (trains/moco_engine.py, trains/simsiam_engine.py): a training step runs
eagerly on its first two calls (they size every workspace), is recorded into a hipGraph on the third and replayed from then on - on
one GPU and, with the RCCL backend, on N GPUs too (the collectives are captured with the kernels; CETPICK_DIST_GRAPH=0 keeps the N>1
step eager, and a capture that fails on any rank falls back to the eager step on every rank).

An engine supplies `_step_eager(inputs)` (inputs: {name: device tensor}), registers its pre-cut weight images in `self._images`
(hipops.WeightImages) and keeps its gradient exchange and its meters; the driver owns the learning-rate scalar, the capture, the
replay, the weight-image version check and the tear-down.
"""
import ctypes
import os
import warnings

import torch

from .. import _lib as L
from .. import hipops as H


def _dist():
    import torch.distributed as dist
    return dist if (dist.is_available() and dist.is_initialized()) else None


def _drain_watchdog():
    """Data parallel, before a capture: wait until the process group's watchdog thread holds no Work of the eager steps.
    The watchdog polls its list every 100 ms (hipEventQuery on each Work's end event) and drops the Works it finds
    complete.  A Work of the eager warm-up steps that is still on that list when the capture starts gets polled DURING
    the capture - and ProcessGroupNCCL's internal communication stream, on which that end event was recorded, is by then
    part of the capture: ROCm answers hipErrorCapturedEvent ("operation not permitted on an event last recorded in a
    capturing stream") for an event whose stream is capturing NOW, the watchdog rethrows and the process aborts
    (profiles/r04_watchdog_abort.txt: 1 run in ~10; `thread_local` capture mode cured the other form of this race, the
    query of an unrelated event under `global` mode).
    The drain is a synchronisation, not a timer: the caller has synchronised the device (every Work is complete), and
    `ProcessGroup._wait_for_pending_works()` (c10d: ProcessGroupNCCL::waitForPendingWorks) returns once it has seen, under
    the watchdog's own two mutexes, BOTH the watchdog's work list and its completed-work list empty - it re-checks every
    watchdog poll period until then.  Nothing is issued between that return and the capture, so the list is still empty
    when the capture begins, and every collective of the captured step is synchronous (no Work is registered under
    capture).  Paid once per capture, never per step.  Only a torch build without the binding falls back to waiting
    three poll periods (CETPICK_WATCHDOG_DRAIN_S, default 0.3 s) - and says so."""
    pg = _dist().distributed_c10d._get_default_group()
    wait = getattr(pg, "_wait_for_pending_works", None)
    if wait is not None:
        wait()
        return
    import time
    warnings.warn("this torch has no ProcessGroup._wait_for_pending_works: draining the watchdog by a timed wait")
    time.sleep(float(os.environ.get("CETPICK_WATCHDOG_DRAIN_S", "0.3")))


class StepGraph:
    WARMUP = 2                      # eager calls in front of the capture
    GRAPH_OUTPUTS = ("loss",)       # attributes the step sets: a replay points them back at the captured step's tensors

    def __init__(self, module, arenas, lr, weight_decay, use_graph):
        self._module = module        # whose buffers broadcast_state() sends
        self._arenas = arenas        # the ParamArenas the step trains: their versions are part of the weight-image check
        self.lr, self.weight_decay = float(lr), float(weight_decay)
        dev = arenas[0].flat.device
        self.lr_dev = torch.full((1,), self.lr, dtype=torch.float32, device=dev)
        d = _dist()
        self.world = d.get_world_size() if d else 1
        self.dist_on = H._distributed()
        # an eager N>1 step is launch-bound on the host (3.5 ms against 2.4 ms on one GPU, before any collective); RCCL
        # collectives can be captured into the graph, gloo's (host-side) cannot
        graph_ok = (not self.dist_on) or (d.get_backend() == "nccl" and os.environ.get("CETPICK_DIST_GRAPH", "1") != "0")
        self.use_graph = bool(use_graph) and graph_ok and dev.type == "cuda"      # (read on every call: bench.py flips it)
        self._graph = None
        self._static = None
        self._calls = 0
        self._images = None          # the engine's hipops.WeightImages (None: no pre-cut images)
        self._img_versions = None

    def set_lr(self, lr):
        """utils/utils.py:58-70 `adjust_learning_rate` target: the schedule reaches a captured graph
        through a device scalar."""
        self.lr = float(lr)
        self.lr_dev.fill_(self.lr)

    def broadcast_state(self, src=0):
        """Identical replicas before the first step (what DistributedDataParallel does at construction): the flat parameter
        arenas (the parameters themselves are kernel-layout views, which RCCL refuses as non-contiguous) and the buffers."""
        d = _dist()
        if d is None:
            return
        for a in self._arenas:
            d.broadcast(a.flat, src)
        for b in self._module.buffers():
            d.broadcast(b, src)
        self.refresh_weight_images()

    # ---- pre-cut weight images -----------------------------------------------------------------------------------------
    def _weight_versions(self):
        """Changes whenever a torch op wrote a cached weight OR a flat arena (dist.broadcast, arena.flat.copy_, a checkpoint
        load): the engine's own optimizer / EMA kernels go through the C-ABI, bump nothing, and refresh by themselves."""
        return self._images.versions() + sum(a.flat._version for a in self._arenas)

    def refresh_weight_images(self):
        """Call after writing the weights from outside the step (checkpoint load, broadcast): the step itself keeps the images
        current, and notices writes made through torch ops by their version counters."""
        if self._images is not None:
            self._images.refresh_all()
            self._img_versions = self._weight_versions()

    # ---- capture and replay --------------------------------------------------------------------------------------------
    def _capture(self, inputs):
        """Record one step into a hipGraph.  Returns the graph, or None when the data-parallel ranks agreed to stay
        eager.  With collectives in the step every rank must take the same decision: a rank that replays a graph
        and a rank that launches eagerly no longer issue their collectives in one order."""
        self._static = {k: v.clone() for k, v in inputs.items()}
        torch.cuda.synchronize()
        if self.dist_on:
            _drain_watchdog()
        graph = torch.cuda.CUDAGraph(keep_graph=True)      # the hipGraph_t stays queryable (node_counts)
        err = None
        try:
            # Data parallel: the process group's watchdog THREAD polls (hipEventQuery) Works at its own pace.  Two races, two
            # cures: (1) under the default "global" capture mode ANY such call from another thread while this one is
            # capturing terminates the process (hipErrorStreamCaptureUnsupported) - "thread_local" restricts only the capturing
            # thread; (2) a query of an event whose own stream has joined the capture fails in either mode
            # (hipErrorCapturedEvent) - _drain_watchdog() above emptied the watchdog's list, and nothing captured adds to it.
            mode = "thread_local" if self.dist_on else "global"
            # (the capture runs on a stream of its own: the kept-clean workspaces the eager steps made for THEIR stream get a twin for it
            # now, or their zero-fill would be recorded and replay with every step)
            cap = torch.cuda.Stream(device=self.lr_dev.device)
            L.prime_workspaces_for_stream(torch.cuda.current_stream(), cap)
            with torch.cuda.graph(graph, stream=cap, capture_error_mode=mode):       # records, does not execute
                self._step_eager(self._static)
        except Exception as e:                        # e.g. a collective that cannot be captured
            if not self.dist_on:
                raise
            err = e
        # the graph bakes in the addresses of the weight-gradient slab buffers: they must never be reallocated from now on
        for a in self._arenas:
            for prm in a.params:
                if getattr(prm, "_mi_slabs", None) is not None:
                    prm._mi_slabs_pinned = True
        if self.dist_on:
            # the outcome is agreed on eagerly (outside any capture); a stream or communicator left in an error
            # state by the aborted capture surfaces here instead of being swallowed
            torch.cuda.synchronize()
            ok = torch.tensor([0 if err is not None else 1], dtype=torch.int32, device=self.lr_dev.device)
            _dist().all_reduce(ok, op=_dist().ReduceOp.MIN)
            if int(ok.item()) == 0:
                warnings.warn("hipGraph capture of the data-parallel step failed on %s (%s); every rank runs it eagerly"
                              % ("this rank" if err is not None else "another rank", err))
                del graph
                self.use_graph = False
                self._static = None
                return None
        self._graph_out = [getattr(self, a) for a in self.GRAPH_OUTPUTS]
        return graph

    def _run(self, inputs, eager=False):
        """Returns the loss as a 0-d device tensor (no host sync).

        Graph mode: the first WARMUP calls run eagerly, the next one captures the step into a hipGraph and from then on each
        call is one graph replay.  A batch whose shapes differ from the captured one (a short last batch) runs eagerly; under
        data parallelism it is an error (every rank has to take the same path)."""
        if self._images is not None and self._weight_versions() != self._img_versions:
            self.refresh_weight_images()               # first step, or the weights / arenas were written through torch ops
        if eager or not self.use_graph:
            return self._step_eager(inputs)
        if self._graph is None:
            self._calls += 1
            if self._calls <= self.WARMUP:
                return self._step_eager(inputs)
            self._graph = self._capture(inputs)
            if self._graph is None:
                return self._step_eager(inputs)
        st = self._static
        if inputs.keys() != st.keys() or any(v.shape != st[k].shape for k, v in inputs.items()):
            if self.dist_on:
                raise ValueError("data-parallel graph step: batch %s differs from the captured %s (use drop_last)"
                                 % ({k: tuple(v.shape) for k, v in inputs.items()}, {k: tuple(v.shape) for k, v in st.items()}))
            return self._step_eager(inputs)
        if len(st) == 2:
            a, b = st
            H.copy_pair_(st[a], inputs[a], st[b], inputs[b])      # (one launch for both views)
        else:
            for k, v in inputs.items():
                st[k].copy_(v)
        H._bump_weight_epoch()                          # the replayed optimizer kernels write the arenas (no Python runs)
        self._graph.replay()
        for a, v in zip(self.GRAPH_OUTPUTS, self._graph_out):
            setattr(self, a, v)
        return self.loss

    def node_counts(self):
        """{'kernel', 'memcpy', 'memset', 'other'} nodes of the captured step (None while the step runs eagerly)."""
        if self._graph is None:
            return None
        counts = (ctypes.c_int * 4)()
        L.call("mi_graph_node_counts", ctypes.c_void_p(self._graph.raw_cuda_graph()), ctypes.cast(counts, ctypes.c_void_p))
        return dict(zip(("kernel", "memcpy", "memset", "other"), [int(c) for c in counts]))

    def close(self):
        """Release everything that refers to the process group's communicator BEFORE the group is destroyed: the
        captured hipGraph holds the RCCL kernels of its collectives, so it has to go first; then the device is drained.
        The parameters lose the second-gradient views only this engine's optimizer reads (hipops._grad_target).
        Call before dist.destroy_process_group()."""
        if self._graph is not None:
            torch.cuda.synchronize()
            self._graph.reset()
            self._graph = None
        self._static = None
        self._calls = 0
        for a in self._arenas:
            a.drop_second_grads()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
