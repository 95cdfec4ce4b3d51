"""One SimSiam training step as the reference's hot loop performs it (trains/base_trainer.py:486-508 ->
ModelWithLossSimSiam.forward :124-133 -> models/networks/simsiam_model_2d.py:776-819 two-view forward ->
trains/tomo_simsiam_trainer.py:28-40 loss -> zero_grad / backward / SGD step, simsiam_main.py:65), driven without per-iteration
host work and replayed from a hipGraph (round 6):

  * the model's parameters live in one flat fp32 arena (hipops.ParamArena) with TWO gradient arenas: both views run through the same
    weights, so every parameter receives two gradient contributions per step - the first is written into arena A, the second into
    arena B (no `grad.add_` launch per parameter, ~60 a step), and ONE fused kernel applies p -= lr (gA + gB) (mi_sgd_step2) instead of
    torch.optim.SGD's per-tensor loop;
  * the pre-cut weight images of the 3 x 3 layers (csrc/conv_p2d.hip: forward and data-gradient image per convolution) are kept in a
    hipops.WeightImages group and re-cut by two launches behind the SGD kernel - not by one launch in front of each of the 48
    direct-kernel calls;
  * the loss meters (loss, cosine_loss, output_std) are accumulated on the device by one launch inside the step and read once per
    print interval;
  * the whole step - two forwards, loss, backward, optimizer, image refresh, meters - is captured into a hipGraph on the third call and
    replayed from then on (trains/step_graph.py; RCCL collectives are captured with it, gloo ranks stay eager).

Data-parallel ranks exchange the two gradient arenas (bucketed all-reduce, RCCL over xGMI) between backward and the optimizer kernel,
whose grad_scale carries the 1 / world of DistributedDataParallel's averaging; SyncBN statistics are exchanged by the BatchNorm
modules themselves.
"""
import torch

from .. import hipops as H
from .step_graph import StepGraph


class SimSiamStepEngine(StepGraph):
    STAT_KEYS = ("loss", "cosine_loss", "output_std")
    GRAPH_OUTPUTS = ("loss", "stats")

    def __init__(self, model_with_loss, lr, weight_decay=0.0, use_graph=False, n_buckets=2):
        self.mwl = model_with_loss
        self.model = model_with_loss.model
        self.arena = H.ParamArena(self.model, second_grad_arena=True)
        super().__init__(self.model, [self.arena], lr, weight_decay, use_graph)
        dev = self.arena.flat.device
        self._one = torch.ones((), dtype=torch.float32, device=dev)
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.stat_sums = torch.zeros(4, dtype=torch.float32, device=dev)
        self.stats = {}
        n = self.arena.numel
        per = (max((n + n_buckets - 1) // n_buckets, 1 << 18) + 3) // 4 * 4
        self.buckets = [(a, min(a + per, n)) for a in range(0, n, per)]
        self._images = self._build_weight_images()

    # ---- pre-cut weight images of the 3 x 3 / stride-1 convolutions (conv_p2d.hip) -----------------------------------
    def _build_weight_images(self):
        """Group "p2d": forward + data-gradient image of every 3 x 3 / stride-1 C -> C convolution, re-cut behind the SGD kernel."""
        if not self.arena.flat.is_cuda:
            return None
        imgs = H.WeightImages()
        for m in self.model.modules():
            if isinstance(m, H.HipConv2d) and m.ci == m.co and m.k == 3 and m.stride == 1 and m.pad == 1 and m.co in (64, 128, 256) \
                    and H._phys_ok(m.weight):
                imgs.add("p2d", "p2d", m.weight, False)
                imgs.add("p2d", "p2d", m.weight, True)
        return imgs

    # ---- the step ------------------------------------------------------------------------------------------------
    def _exchange(self):
        """Sum both gradient arenas over the ranks (the averaging rides in the optimizer kernel)."""
        for flat in (self.arena.flat_grad, self.arena.flat_grad2):
            for a, b in self.buckets:
                H.dist_all_reduce(flat[a:b])

    def _step_eager(self, batch):
        self.arena.zero_grad()
        H.ACTIVE_IMAGES = self._images                 # the cached weight images are valid inside the step only
        try:
            _, loss, stats = self.mwl(batch, 0, "train")
            loss.backward(self._one)
        finally:
            H.ACTIVE_IMAGES = None
        self.arena.settle_grads()
        if self.dist_on:
            self._exchange()
        H.sgd_step2_(self.arena.flat, self.arena.flat_grad, self.arena.flat_grad2, self.lr, self.weight_decay, self.lr_dev,
                     grad_scale=1.0 / self.world)
        if self._images is not None:
            self._images.refresh("p2d")
        keys = [k for k in self.STAT_KEYS if k in stats]
        H.scalar_accumulate_(self.stat_sums, *[stats[k].detach().reshape(()) for k in keys])
        self._stat_keys = keys
        self.loss = loss.detach()
        self.stats = stats
        return self.loss

    def step_eager(self, x1, x2):
        return self._run({"input": x1, "input_aug": x2}, eager=True)

    def step(self, x1, x2):
        return self._run({"input": x1, "input_aug": x2})

    def step_batch(self, batch):
        return self._run({k: v for k, v in batch.items() if isinstance(v, torch.Tensor)})

    def take_stat_sums(self):
        """{key: sum over the steps since the last call} (one host read), and reset."""
        v = self.stat_sums.tolist()
        self.stat_sums.zero_()
        return dict(zip(getattr(self, "_stat_keys", self.STAT_KEYS), v))
