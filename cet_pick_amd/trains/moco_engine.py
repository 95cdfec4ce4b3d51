"""One MoCo training step as the reference's hot loop performs it
(trains/base_trainer.py:486-508 -> models/moco.py:101-146 -> trains/tomo_moco_trainer.py:73 ->
optimizer.step), driven without per-iteration host syncs and replayed from a hipGraph (trains/step_graph.py) - on one GPU and,
with the RCCL backend, on N GPUs too.

Data-parallel ranks (one process per GPU, torch.distributed backend "nccl" = RCCL) exchange per step:
gradient arena all-reduce (40.4 MB fp32), MoCo key all-gather (B x 128), SyncBN per-channel sums.
"""
import os

import torch

from .. import hipops as H
from .step_graph import StepGraph


class MocoStepEngine(StepGraph):
    def __init__(self, moco, lr, weight_decay=0.0, use_graph=False):
        self.moco = moco
        self.arena_q, self.arena_k = moco.flatten_parameters()
        super().__init__(moco, [self.arena_q, self.arena_k], lr, weight_decay, use_graph)
        dev = self.arena_q.flat.device
        self.logits = None
        self._one = torch.ones((), dtype=torch.float32, device=dev)
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)
        self._loss_buf = self.loss
        # running sum of the steps' losses since take_loss_sum(): accumulated by one launch INSIDE the step (a graph node) - run_epoch's
        # meters read it at print time instead of launching a mean and an add behind every step
        self.loss_sum = torch.zeros((), dtype=torch.float32, device=dev)
        self._xchg = None                # side stream of the gradient exchange (overlaps the backward pass)
        self.buckets_sent = []           # tags of the last step's exchanges, in issue order (tests / diagnostics)
        if self.dist_on:
            self._setup_buckets()
        # weight gradients of layer1-3 and the head on a side stream, one fork per stage (hipops.SIDE_WGRADS)
        self.side_wgrads = dev.type == "cuda" and os.environ.get("CETPICK_SIDE_WGRADS", "1") != "0"
        self._wside = None
        self._wside_used = False
        self._wside_keep = []
        if self.side_wgrads:
            moco.encoder_q.grad_marker = self._on_marker
        self._images = self._build_weight_images()

    # ---- pre-cut weight images of the layer1 convolutions (conv_direct3.hip) ---------------------------------
    def _build_weight_images(self):
        """Group "q": forward + data-gradient images of encoder_q's 64 -> 64 3^3 convolutions (re-cut behind the SGD
        kernel), group "k": forward images of encoder_k's (re-cut behind the EMA kernel) - one launch each per step
        instead of one image build in front of each of the 12 direct-kernel launches."""
        if not self.arena_q.flat.is_cuda:
            return None
        imgs = H.WeightImages()
        for enc, group in ((self.moco.encoder_q, "q"), (self.moco.encoder_k, "k")):
            for m in enc.modules():
                if isinstance(m, H.HipConv3d) and H.WeightImages.eligible(m.weight, m.k, m.stride, m.pad):
                    imgs.add(group, "direct", m.weight, False)
                    if group == "q":
                        imgs.add(group, "direct", m.weight, True)
            # the stride-2 block fronts (conv_s2.hip): forward image per encoder, data-gradient image for encoder_q
            for blk in enc.modules():
                ds = getattr(blk, "downsample", None)
                if ds is None or getattr(blk, "stride", 1) != 2 or not hasattr(blk, "conv1"):
                    continue
                w, wds = blk.conv1.weight, ds[0].weight
                co, ci = int(w.shape[0]), int(w.shape[1])
                if (co, ci) not in ((128, 64), (256, 128)) or not (H._phys_ok(w) and H._phys_ok(wds)):
                    continue
                imgs.add(group, "s2", w, False, wds)
                if group == "q":
                    imgs.add(group, "s2", w, True, wds)
        self.moco.weight_images = imgs                 # MoCo re-cuts group "k" right behind its momentum update
        return imgs

    # ---- data parallel: bucketed gradient all-reduce overlapped with the backward pass ---------------------
    def _setup_buckets(self):
        """Arena ranges whose gradients are complete at each stage boundary of the backward pass (parameters sit in
        the arena in registration order: stem, layer1, layer2, layer3, feature_3d, fc, heads)."""
        enc = self.moco.encoder_q
        first = {}
        for (name, _), off in zip(enc.named_parameters(), self.arena_q.offsets):
            first.setdefault(name.split(".")[0], off)
        end = self.arena_q.numel
        l1, l2, l3 = first["layer1"], first["layer2"], first["layer3"]
        # marker tag -> range that is final when the gradient of that stage's INPUT exists
        self._bucket = {"layer3": (l3, end), "layer2": (l2, l3), "layer1": (l1, l2), "stem": (0, l1)}
        enc.grad_marker = self._on_marker

    def _reduce_bucket(self, tag):
        """One bucket of the gradient arena goes out on the exchange stream: forked from the stream the backward pass is
        on (this runs in an autograd hook, i.e. right behind the last kernel that wrote the bucket), joined again before
        the optimizer step.  The collective itself is issued synchronously - its internal wait only holds the exchange
        stream - because an async Work under hipGraph capture kills the process-group watchdog (hipops.dist_all_reduce)."""
        a, b = self._bucket[tag]
        H.flush_wgrad_reduces()                       # the bucket's weight gradients still sit in split-K slabs
        # (with the weight gradients on their side stream the slabs of the stage were reduced there, behind the launches
        # that wrote them: the exchange stream then waits for both)
        if b > a and not self.arena_q.flat_grad.is_cuda:        # (CPU tensors over gloo: plumbing tests)
            H.dist_all_reduce(self.arena_q.flat_grad[a:b])
            self.buckets_sent.append(tag)
        elif b > a:
            cur = torch.cuda.current_stream()
            if self._xchg is None:
                self._xchg = torch.cuda.Stream(device=self.arena_q.flat_grad.device)
            self._xchg.wait_stream(cur)
            if self._wside_used:
                self._xchg.wait_stream(self._wside)
            with torch.cuda.stream(self._xchg):
                H.dist_all_reduce(self.arena_q.flat_grad[a:b])
            self.buckets_sent.append(tag)

    def _on_marker(self, tag):
        if self.side_wgrads and tag in ("layer3", "layer2", "layer1"):
            self._issue_side_wgrads(enqueue=(tag == "layer3"))
        if self.dist_on:
            self._reduce_bucket(tag)

    def _issue_side_wgrads(self, enqueue=False):
        """The data-gradient chain has left a stage: its collected weight-gradient launches go out on the side stream (one
        fork), next to the following stage's kernels on the main stream.  The deferred key enqueue rides along behind
        layer3's: the backward pass read the queue for the last time in the logits' gradient, long before."""
        items = H.SIDE_WGRADS
        if not items:
            return
        cur = torch.cuda.current_stream()
        if H.PROFILE is not None:                      # bench.py's roofline pass: every call timed by itself, in line
            H.run_wgrad_jobs(items)
            H.flush_wgrad_reduces()
            if enqueue:
                self.moco.flush_enqueue()
            del items[:]
            return
        if self._wside is None:
            self._wside = torch.cuda.Stream(device=self.arena_q.flat_grad.device)
        self._wside.wait_stream(cur)
        with torch.cuda.stream(self._wside):
            H.run_wgrad_jobs(items)                   # (convolutions of one geometry: one launch for the group)
            H.flush_wgrad_reduces()                   # the stage's split-K slabs, behind the launches that wrote them
            if enqueue:
                self._wside_keep.append(self.moco._pending_keys)
                self.moco.flush_enqueue()
        # the launches read activations / gradients allocated on the main stream: they stay referenced until the join, so
        # that the allocator cannot hand their memory to the main stream's next kernels while the side stream reads it
        self._wside_keep.extend(items)
        del items[:]
        self._wside_used = True

    # ---- the step ------------------------------------------------------------------------------------------------
    def step(self, im_q, im_k):
        """Returns the loss as a 0-d device tensor (no host sync); graph mode: StepGraph._run."""
        return self._run({"q": im_q, "k": im_k})

    def step_eager(self, im_q, im_k):
        return self._run({"q": im_q, "k": im_k}, eager=True)

    def _step_eager(self, inputs):
        im_q, im_k = inputs["q"], inputs["k"]
        moco = self.moco
        self.buckets_sent = []
        self.arena_q.zero_grad()
        H.ACTIVE_IMAGES = self._images                 # the cached weight images are valid inside the step only
        moco.defer_enqueue = True                      # the backward reads the queue in place; keys go in behind it
        try:
            H.stamp("step:start")
            logits, labels = moco(im_q, im_k)
            self.logits = logits.detach()              # (B, 1 + r) of the last step; under graph replay a static buffer
            loss = H.cross_entropy_label0(logits, out=self._loss_buf)      # lands in the engine's loss buffer: no copy
            H.DEFERRED_WGRADS = [] if self.arena_q.flat_grad.is_cuda else None     # split-K slabs of the wgrads: one reduce
            H.SIDE_WGRADS = [] if self.side_wgrads else None
            self._wside_used = False
            loss.backward(self._one)                   # (a kept seed: autograd's ones_like(loss) is a fill launch per step)
            if H.SIDE_WGRADS:                          # collected behind the last stage boundary: in line
                H.run_wgrad_jobs(H.SIDE_WGRADS)
            H.SIDE_WGRADS = None
            if self._wside_used:
                torch.cuda.current_stream().wait_stream(self._wside)
            del self._wside_keep[:]
            H.stamp("backward:end")
            H.flush_wgrad_reduces()
            moco.flush_enqueue()
        finally:
            H.DEFERRED_WGRADS = None
            H.SIDE_WGRADS = None
            H.ACTIVE_IMAGES = None
            moco.defer_enqueue = False
            moco._pending_keys = None
        if self.dist_on:
            # layer3+heads, layer2 and layer1 went out from the autograd hooks while the backward was still running
            # (RCCL over xGMI on its own stream); the stem's gradients are the last to exist
            self._reduce_bucket("stem")
            if self._xchg is not None:
                torch.cuda.current_stream().wait_stream(self._xchg)
        # (flat_grad holds the SUM over the ranks; the 1 / world of DistributedDataParallel's averaging rides in the SGD
        # kernel instead of a pass of its own over the arena)
        H.sgd_step_(self.arena_q.flat, self.arena_q.flat_grad, self.lr, self.weight_decay, self.lr_dev,
                    grad_scale=1.0 / self.world)
        if self._images is not None:
            self._images.refresh("q")                  # next step's forward / data-gradient images of encoder_q
        self.loss_sum.add_(self.loss)
        H.stamp("step:end")
        return self.loss

    def take_loss_sum(self):
        """Sum of the losses of the steps since the last call (one host sync), and reset."""
        v = float(self.loss_sum.item())
        self.loss_sum.zero_()
        return v
