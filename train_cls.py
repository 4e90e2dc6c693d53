#!/usr/bin/env python
"""Classification training loop -- counterpart of /root/reference/train_cls.py (train :52-73, evaluate :92-124, main
:366-480) on the MI355X-native modules: same CLI (``--model --batch_size --lr --momentum --num_points --epochs``),
label-smoothed cross entropy (:31-51), SGD with momentum (:404), per-epoch evaluation.

    python train_cls.py --model pointnet2 --epochs 2            # synthetic clouds when ModelNet40 is not on disk

ModelNet40 is read from ``--data_root`` (``modelnet40_normal_resampled``); without it the same input recipe runs on
synthetic clouds (throughput and plumbing only -- accuracy on random labels means nothing).  Upstream's LR never decays
(``train_cls.py:475`` + ``misc/utils.py:16-19``: the scheduler is built and stepped but its value is not applied);
``--lr_decay`` enables the evident intent (x0.7 every 20 epochs) and is off by default to match.
"""
import argparse
import os
import time

from pointcloudlib_amd.affinity import pin_to_gpu_node

pin_to_gpu_node(int(os.environ.get("LOCAL_RANK", "0")))      # before torch / HIP start threads (pointcloudlib_amd/affinity.py)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pointcloudlib_amd.data_utils.modelnet40_loader import ModelNet40, SyntheticModelNet40
from pointcloudlib_amd.train_utils import loss_backward, make_sgd, soft_cross_entropy_loss


def build_model(name):
    if name == "pointnet":
        from pointcloudlib_amd.networks.cls.pointnet import PointNet as M
    elif name == "pointnet2":
        from pointcloudlib_amd.networks.cls.pointnet2 import PointNet2_cls as M
    elif name == "dgcnn":
        from pointcloudlib_amd.networks.cls.dgcnn import DGCNN as M
    elif name == "pointconv":
        from pointcloudlib_amd.networks.cls.pointconv import PointConvDensityClsSsg as M
    elif name == "pointcnn":
        from pointcloudlib_amd.networks.cls.pointcnn import PointCNNcls as M
    else:
        raise SystemExit(f"unknown --model {name} (pointnet | pointnet2 | dgcnn | pointconv | pointcnn); KPConv is out of scope")
    return M()


def forward(net, name, pts, normals):
    if name in ("pointnet", "dgcnn", "pointconv"):            # train_cls.py:62-63 (pointconv permutes internally upstream)
        return net(pts.transpose(1, 2).contiguous())
    if name == "pointnet2":
        return net(pts, normals)                               # :65-66
    return net(pts)


def lookahead(loader, dev):
    """(batch on the device, next batch on the device or None): the next batch's sampling can be issued one step ahead."""
    it = iter(loader)
    cur = next(it, None)
    cur = None if cur is None else tuple(t.to(dev) for t in cur)
    while cur is not None:
        nxt = next(it, None)
        nxt = None if nxt is None else tuple(t.to(dev) for t in nxt)
        yield cur, nxt
        cur = nxt


def run_epoch(net, name, loader, dev, optimizer=None, side=None, fnet=None):
    """One pass over ``loader``; ``fnet``: a frozen evaluator of ``net`` (pointcloudlib_amd.inference) that runs the validation forwards."""
    train = optimizer is not None
    model = net if train or fnet is None else fnet
    net.train(train)
    seen = correct = 0
    loss_sum = 0.0
    prefetch = side is not None and hasattr(net, "precompute_sampling")
    pending = None
    t0 = time.perf_counter()
    for (pts, normals, labels), nxt in lookahead(loader, dev):
        with torch.set_grad_enabled(train):
            if prefetch:
                cur_samp = pending
                # FPS / ball query of the NEXT batch on the library's side stream, beside this step (enqueued ahead of the forward:
                # bench.py measured 1.900 vs 1.914 ms for enqueueing it behind the forward)
                pending = net.precompute_sampling(nxt[0], stream=side) if nxt is not None else None
                out = model(pts, normals, sampling=cur_samp)
            else:
                out = forward(model, name, pts, normals)
            if train:
                loss = soft_cross_entropy_loss(out, labels)
                optimizer.zero_grad(set_to_none=True)
                loss_backward(loss)                            # optimizer.step(loss), train_cls.py:404: backward + update
                optimizer.step()
                loss_sum += loss.item() * len(labels)
        correct += int((out.argmax(1) == labels).sum())
        seen += len(labels)
    torch.cuda.synchronize()
    return correct / max(seen, 1), loss_sum / max(seen, 1), seen / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="pointnet2")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--num_points", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--data_root", default=None)
    ap.add_argument("--lr_decay", action="store_true")
    ap.add_argument("--synthetic_items", type=int, default=512)
    ap.add_argument("--seed", type=int, default=0, help="numpy (shuffles, augmentation: freeze_random_seed, train_cls.py:27-28) and torch (init)")
    ap.add_argument("--fast_eval", action="store_true", help="--model pointnet2 | pointnet: validation through pointcloudlib_amd.inference (frozen(net) | FrozenPointNet(net))")
    a = ap.parse_args()
    if a.fast_eval and a.model not in ("pointnet2", "pointnet"):
        raise SystemExit("--fast_eval: --model pointnet2 or pointnet only")
    if not torch.cuda.is_available():
        raise SystemExit("train_cls.py needs a GPU (the HIP path has no CPU fallback)")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        # the reference driver is single-process (train_cls.py:54-75); this one has no gradient exchange wired in, so N copies
        # under torchrun would train N unrelated replicas on cuda:0.  The data-parallel step lives in bench.py / dp.py.
        raise SystemExit("train_cls.py is a single-process driver: do not launch it under torchrun (WORLD_SIZE > 1)")
    dev = torch.device("cuda")
    try:
        train_set = ModelNet40(a.num_points, True, a.batch_size, shuffle=True, root=a.data_root)
        val_set = ModelNet40(a.num_points, False, a.batch_size, shuffle=False, root=a.data_root)
    except FileNotFoundError as e:
        print(f"[train_cls] {e}\n[train_cls] -> synthetic clouds")
        train_set = SyntheticModelNet40(a.num_points, True, a.batch_size, shuffle=True, n_items=a.synthetic_items)
        val_set = SyntheticModelNet40(a.num_points, False, a.batch_size, n_items=max(a.batch_size, a.synthetic_items // 4), seed=1)
    np.random.seed(a.seed)
    torch.manual_seed(a.seed)
    net = build_model(a.model).to(dev)
    opt = make_sgd(net.parameters(), lr=a.lr, momentum=a.momentum)
    side = "own" if a.model == "pointnet2" else None     # sampling of batch t+1 beside batch t, on the network's private stream
    fnet = None
    if a.fast_eval:
        from pointcloudlib_amd.inference import FrozenPointNet, frozen
        fnet = FrozenPointNet(net) if a.model == "pointnet" else frozen(net)
    best = 0.0
    for epoch in range(a.epochs):
        if a.lr_decay and epoch and epoch % 20 == 0:
            for g in opt.param_groups:
                g["lr"] *= 0.7
        acc, loss, rate = run_epoch(net, a.model, train_set, dev, opt, side)
        vacc, _, vrate = run_epoch(net, a.model, val_set, dev, None, side, None if fnet is None else fnet.refresh())
        best = max(best, vacc)
        print(f"epoch {epoch}: train loss {loss:.3f} acc {100 * acc:.2f} ({rate:.0f} clouds/s)   val acc {100 * vacc:.2f} "
              f"(best {100 * best:.2f}, {vrate:.0f} clouds/s)", flush=True)


if __name__ == "__main__":
    main()
