"""Host-side drop-in surface that needs no GPU: flags, lr schedule, checkpoint layout, factory."""
import json
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def test_opts_defaults_and_derived_fields(tmp_path, monkeypatch):
    from cet_pick_amd.opts import opts
    monkeypatch.chdir(tmp_path)
    o = opts().parse(["moco", "--arch", "moco3d_18", "--batch_size", "64", "--gpus", "0,1", "--lr_step", "90,120",
                      "--debug", "0"])
    assert o.task == "moco" and o.arch == "moco3d_18" and o.gpus == [0, 1] and o.gpus_str == "0,1"
    assert o.lr_step == [90, 120] and o.seed == 317 and o.K == 200 and o.nms == 3 and o.dog == [2.5, 5]
    assert o.dist_backend == "nccl" and o.dist_url == "env://" and o.chunk_sizes == [32, 32]
    assert o.save_dir == os.path.join(str(tmp_path), "exp", "moco", "default")
    assert o.fix_res is True and o.cutoff_z == 10 and o.out_thresh == 0.25 and o.order == "xzy"
    o2 = opts().parse(["simsiam3d", "--dog", "3,5", "--resume"])
    assert o2.head_conv == 128 and o2.dog == [3.0, 5.0]
    assert o2.load_model.endswith(os.path.join("exp", "simsiam3d", "default", "model_last.pth"))
    assert opts().parse(["semi", "--gpus", "-1"]).gpus == [-1]
    o3 = opts().parse(["semi", "--warm", "--cosine"])       # the reference raises NameError here
    assert 0 < o3.warmup_to <= o3.lr
    o4 = opts().init(["moco"])
    assert o4.heads == {"proj": 256, "pred": 256} and o4.input_h == 32 and o4.dataset == "moco"
    o5 = opts().init(["semi"])
    assert o5.heads == {"hm": 1, "proj": 32} and o5.output_h == 32


def test_lr_schedule_matches_reference(golden):
    from cet_pick_amd.utils.utils import adjust_learning_rate

    class A:
        lr, lr_decay_rate, num_epochs, lr_step = 0.02, 0.1, 140, [90, 120]
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.02)
    for cosine, ep, lr in golden("lr_sched.npz")["rows"]:
        A.cosine = bool(cosine)
        adjust_learning_rate(A, opt, int(ep))
        assert abs(opt.param_groups[0]["lr"] - lr) < 1e-12


def test_factory_and_checkpoint_layout(tmp_path, capsys):
    from cet_pick_amd.models.model import create_model, save_model, load_model
    heads = {"proj": 256, "pred": 256}
    m = create_model("moco3d_18", heads, 0, last_k=3, local_path=None)      # kwargs the reference passes
    keys = json.load(open(os.path.join(HERE, "golden", "ckpt_keys.json")))["moco3d_encoder"]
    sd = m.state_dict()
    assert list(sd) == list(keys) and all(list(sd[k].shape) == keys[k] for k in keys)
    assert m.proj is m.pred
    path = str(tmp_path / "model_last.pth")
    save_model(path, 7, m)
    ck = torch.load(path)
    assert set(ck) == {"epoch", "state_dict"} and ck["epoch"] == 7
    assert all(v.is_contiguous() for v in ck["state_dict"].values())
    # a DataParallel/DDP-style checkpoint ('module.' prefix), one wrong shape and one stray key
    ck2 = {"epoch": 3, "state_dict": {"module." + k: v for k, v in ck["state_dict"].items()}}
    ck2["state_dict"]["module.fc.bias"] = torch.zeros(7)
    ck2["state_dict"]["module.not_there"] = torch.zeros(1)
    torch.save(ck2, path)
    m2 = create_model("moco3d_18", heads, 0)
    before = m2.fc.bias.detach().clone()
    m2 = load_model(m2, path)
    out = capsys.readouterr().out
    assert "Skip loading parameter fc.bias" in out and "Drop parameter not_there" in out
    assert torch.equal(m2.fc.bias, before)
    assert torch.equal(m2.conv1.weight.detach(), m.conv1.weight.detach())
    assert m2.conv1.weight.stride() == m.conv1.weight.stride()            # kernel layout survives loading
    with pytest.raises(NotImplementedError):
        create_model("res_18", {"hm": 1}, 64)                             # exists in the reference, outside the hot path


@pytest.mark.parametrize("plane", [512, 1024, 2048])
@pytest.mark.parametrize("head_conv", [32, 64])
def test_head_z_slabs_keep_every_operand_under_the_offset_limit(plane, head_conv):
    """The detector's 3-D head at inference (unet_small.head_z_slabs): every launch's operand - the slab with its halo, of the
    widest of the 32-channel feature map and the head_conv-channel layers - stays under the kernels' 0x7fff0000-byte limit, and
    the slabs tile [0, d) of every batch item exactly once, with the three-plane halo clipped at the volume's ends."""
    from cet_pick_amd.models.networks.unet_small import HEAD_OPERAND_LIMIT, head_z_slabs
    assert HEAD_OPERAND_LIMIT == 0x7fff0000
    hh = ww = plane // 2                                  # the stride-2 stem: the feature plane is half the tomogram's
    plane_bytes = 4 * hh * ww * max(32, head_conv)
    for d in (1, 63, 64, 65, 70, 200, 512):
        for b in (1, 2):
            launches = head_z_slabs(b, d, plane_bytes)
            if b * d * plane_bytes < HEAD_OPERAND_LIMIT:
                assert launches is None, (plane, head_conv, d, b)
                continue
            assert launches, (plane, head_conv, d, b)
            covered = {i: [] for i in range(b)}
            for i, z0, n, lo, hi in launches:
                assert 0 <= i < b and n >= 1
                assert (lo, hi) == (max(0, z0 - 3), min(d, z0 + n + 3))
                assert (hi - lo) * plane_bytes < HEAD_OPERAND_LIMIT, (plane, head_conv, d, b, z0, n)
                covered[i].append((z0, n))
            for i, runs in covered.items():
                ends = [0]
                for z0, n in runs:
                    assert z0 == ends[-1]
                    ends.append(z0 + n)
                assert ends[-1] == d, (plane, head_conv, d, b, i)
    # the smallest head launch - one plane and its halo - of a 2048^2 feature plane at 64 channels no longer fits: refused
    from cet_pick_amd._lib import HipExtensionError
    with pytest.raises(HipExtensionError, match="0x7fff0000"):
        head_z_slabs(1, 64, 4 * 2048 * 2048 * 64)
    assert head_z_slabs(1, 1, 4 * 2048 * 2048 * 64) is None                # (one such plane alone is a 1 GiB operand)


def test_head_z_slabs_forced_slab():
    """`head_slab` forces slabs where the volume fits (the GPU test pins slabbed against whole-volume outputs with it)."""
    from cet_pick_amd.models.networks.unet_small import head_z_slabs
    assert head_z_slabs(1, 29, 4 * 32 * 32 * 32) is None
    assert head_z_slabs(1, 29, 4 * 32 * 32 * 32, slab=8) == [(0, 0, 8, 0, 11), (0, 8, 8, 5, 19), (0, 16, 8, 13, 27),
                                                            (0, 24, 5, 21, 29)]
    assert [t[:3] for t in head_z_slabs(2, 10, 4 * 32 * 32 * 32, slab=8)] == [(0, 0, 8), (0, 8, 2), (1, 0, 8), (1, 8, 2)]


def test_plain_arena_drops_second_gradient_views():
    """A plain ParamArena on a module that a two-arena owner (the SimSiam step engine) flattened before: the second gradient of a
    parameter accumulates into .grad, where the stock optimizer reads it - not into the orphaned second arena."""
    from cet_pick_amd import hipops as H
    m = torch.nn.Linear(4, 3)
    H.ParamArena(m, second_grad_arena=True)
    arena = H.ParamArena(m)
    p = m.weight
    arena.zero_grad()
    for contribution in (1.0, 2.0):
        tgt, acc = H._grad_target(p)
        if acc:
            tgt.add_(torch.full_like(p, contribution))
        else:
            tgt.copy_(torch.full_like(p, contribution))
    assert torch.equal(p.grad, torch.full_like(p, 3.0))
    assert p.grad.data_ptr() == p._mi_grad_view.data_ptr()


def test_grad_into_assigns_routes_and_accumulates():
    """_GradInto over _grad_target, the one way a parameter gradient is written: the first contribution of a step lands in .grad (the
    arena view), the second in the second arena, every further one in a temporary that leaving the block adds onto .grad; the target
    is fixed when the object is made, not when it is entered; a failed launch adds nothing; no parameter, no target."""
    from cet_pick_amd import hipops as H
    m = torch.nn.Linear(4, 3)
    arena = H.ParamArena(m, second_grad_arena=True)
    p = m.weight
    arena.zero_grad()
    first, second, third = H._GradInto(p), H._GradInto(p), H._GradInto(p)      # all made before the first is entered (deferred launches)
    assert (first.accumulates, second.accumulates, third.accumulates) == (False, False, True)
    for dest, value in ((first, 1.0), (second, 2.0), (third, 4.0)):
        with dest as tgt:
            tgt.copy_(torch.full_like(p, value))
    assert first.tgt.data_ptr() == p._mi_grad_view.data_ptr() and second.tgt.data_ptr() == p._mi_grad_view2.data_ptr()
    assert torch.equal(p.grad, torch.full_like(p, 5.0))
    assert torch.equal(p._mi_grad_view2, torch.full_like(p, 2.0))
    with pytest.raises(RuntimeError, match="launch failed"):
        with H._GradInto(p) as tgt:
            tgt.copy_(torch.full_like(p, 8.0))
            raise RuntimeError("launch failed")
    assert torch.equal(p.grad, torch.full_like(p, 5.0))
    with H._GradInto(None) as tgt:
        assert tgt is None
