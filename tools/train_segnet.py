"""Train the SegNet mask network (the reference's vanilla_segmentation/train.py) on the HIP training path.

Same flags and loop as the reference: per epoch a training pass over SegDataset(train list, noise on, --train_length frames; the
reference uses 5000) logging ``CEloss`` per batch, ``model_current.pth`` every 1000 batches, a test pass in eval() over
SegDataset(test list, no noise, --test_length frames; reference 1000) and ``model_{epoch}_{cost}.pth`` on a new best test loss.
Checkpoints are plain state dicts in the reference's key layout.  The optimiser is Adam with the reference's defaults, through
FlatAdam over one flat parameter buffer (df_adam_step); --dataset_config_dir locates train_data_list.txt / test_data_list.txt as
tools/train.py does.

    python tools/train_segnet.py --dataset_root YCB_Video_Dataset --dataset_config_dir datasets/ycb/dataset_config

``--dataset cad_render`` trains a mask network for CAD models with no tree on disk: customCAD scenes rendered on the fly
(datasets/customCAD/online_seg.py, ``RenderedSegDataset``), one class per ``--cad_model`` plus the background, the views and the
renderer under the names of tools/train.py and tools/render_cad_dataset.py.  Batches come channels-last from ``dataset.batch`` over
``dataset.permutation``, fed by ``--workers`` threads, into ``SegNet.forward_nhwc``; the test views follow the training seed range;
``model_current.pth`` is also written after every training pass, and the log ends an epoch with the share of pixels per class.
``--seg_score`` scores the test pass on the device (``df_seg_score`` on the logits the loss reads) and logs ``Test Finish mIoU``.

    python tools/train_segnet.py --dataset cad_render --cad_model a.ply b.ply --backgrounds photos/ --light random
"""
from __future__ import annotations

import argparse
import logging
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from densefusion_amd import train_utils  # noqa: E402
from densefusion_amd.datasets.customCAD import render as cad_render  # noqa: E402
from densefusion_amd.train_utils import FlatAdam, FlatParams  # noqa: E402
from densefusion_amd.vanilla_segmentation.data_controller import SegDataset  # noqa: E402
from densefusion_amd.vanilla_segmentation.loss import Loss  # noqa: E402
from densefusion_amd.vanilla_segmentation.segnet import SegNet  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset_root", type=str, default="", help="dataset root dir (YCB_Video_Dataset)")
    ap.add_argument("--dataset_config_dir", type=str, default="datasets/ycb/dataset_config",
                    help="directory of train_data_list.txt / test_data_list.txt")
    ap.add_argument("--batch_size", type=int, default=3, help="batch size")
    ap.add_argument("--n_epochs", type=int, default=600, help="epochs to train (the loop runs epochs 1 .. n_epochs - 1, as the reference's)")
    ap.add_argument("--workers", type=int, default=10, help="number of data loading workers")
    ap.add_argument("--lr", type=float, default=0.0001, help="learning rate")
    ap.add_argument("--logs_path", type=str, default="logs/", help="path to save logs (unused, as in the reference)")
    ap.add_argument("--model_save_path", type=str, default="trained_models/", help="path to save models")
    ap.add_argument("--log_dir", type=str, default="logs/", help="path to save logs")
    ap.add_argument("--resume_model", type=str, default="", help="resume model name")
    ap.add_argument("--train_length", type=int, default=5000, help="frames per training epoch")
    ap.add_argument("--test_length", type=int, default=1000, help="frames per test pass")
    ap.add_argument("--seed", type=int, default=None, help="random seed (default: drawn, as the reference does)")
    ap.add_argument("--dataset", type=str, default="ycb", choices=("ycb", "cad_render"), help="a YCB-Video tree, or customCAD scenes rendered on the fly")
    cad = ap.add_argument_group("cad_render", "the views and the renderer, under the names of tools/train.py and tools/render_cad_dataset.py")
    cad.add_argument("--cad_model", type=str, nargs="+", default=[], help="PLY mesh(es): model k is class k + 1")
    cad.add_argument("--cad_distractor", type=str, nargs="*", default=[], help="meshes that are drawn and can occlude; background for the loss")
    cad.add_argument("--cad_frames", type=int, default=2000, help="views per training epoch")
    cad.add_argument("--cad_test_frames", type=int, default=200, help="test views: the seed range right after the training range")
    cad.add_argument("--cad_seed", type=int, default=0, help="seed of the first training view")
    cad.add_argument("--cad_fresh", action="store_true", help="fresh views every epoch (the seed range moves on by --cad_frames); default: a fixed set, like a tree")
    cad.add_argument("--seg_height", type=int, default=None, help="window height, a multiple of 32 (default: the largest inside the frame)")
    cad.add_argument("--seg_width", type=int, default=None, help="window width, a multiple of 32 (default: the largest inside the frame)")
    cad.add_argument("--backgrounds", type=str, default=None, help="directory of images that stand behind the objects (default: the grey horizon)")
    cad.add_argument("--seg_blur", type=int, default=1, choices=(0, 1), help="1: the 3 x 3 binomial blur over the composited window")
    cad.add_argument("--seg_noise", type=float, default=5.0, help="sigma of the pixel noise in grey levels (0: none)")
    cad.add_argument("--seg_score", action="store_true", help="score the test pass on the device: log mIoU and per-class IoU (df_seg_score)")
    cad_render.add_view_arguments(cad)
    return ap


def setup_logger(name, path):
    """lib/utils.py's setup_logger: INFO to the file and to stdout, '%(asctime)s : %(message)s'."""
    logger = logging.getLogger(name)
    logger.handlers.clear()
    logger.setLevel(logging.INFO)
    fmt = logging.Formatter("%(asctime)s : %(message)s")
    for h in (logging.FileHandler(path, mode="w"), logging.StreamHandler(sys.stdout)):
        h.setFormatter(fmt)
        logger.addHandler(h)
    return logger


def _clock(st):
    return time.strftime("%Hh %Mm %Ss", time.gmtime(time.time() - st))


def _plain_state_dict(model):
    """The module's state dict as standalone tensors (the parameters are views into the flat buffer of FlatParams)."""
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def cad_datasets(opt):
    """(training set, test set) of --dataset cad_render; the test views follow the last training view --cad_fresh can reach."""
    from densefusion_amd.datasets.customCAD.online_seg import RenderedSegDataset, default_window
    if not opt.cad_model:
        raise SystemExit("--dataset cad_render needs --cad_model")
    h, w = default_window((opt.height, opt.width))
    kw = dict(window=(h if opt.seg_height is None else opt.seg_height, w if opt.seg_width is None else opt.seg_width),
              backgrounds=opt.backgrounds, blur=opt.seg_blur, noise_sigma=opt.seg_noise)
    test_seed = opt.cad_seed + opt.cad_frames * (max(opt.n_epochs - 1, 1) if opt.cad_fresh else 1)
    try:
        return (RenderedSegDataset.from_options(opt, opt.cad_model, opt.cad_distractor, first_seed=opt.cad_seed, frames=opt.cad_frames,
                                                use_noise=True, **kw),
                RenderedSegDataset.from_options(opt, opt.cad_model, opt.cad_distractor, first_seed=test_seed, frames=opt.cad_test_frames,
                                                use_noise=False, **kw))
    except ValueError as e:
        raise SystemExit(f"--dataset cad_render: {e}")


def train_cad(opt):
    """The loop of ``main`` over rendered scenes; returns {"train": per epoch the batch losses, "test": the same, "shares": per epoch
    the class pixel shares of the training pass}; with --seg_score also "miou": per epoch the test pass's mean IoU."""
    dataset, test_dataset = cad_datasets(opt)
    print(len(dataset), len(test_dataset))
    dev = torch.device("cuda", torch.cuda.current_device())
    K = dataset.n_classes
    model = SegNet(label_nbr=K, trainable=True).cuda()
    if opt.resume_model != "":
        model.load_state_dict(torch.load(os.path.join(opt.model_save_path, opt.resume_model), map_location="cuda"))
        for log in os.listdir(opt.log_dir):
            os.remove(os.path.join(opt.log_dir, log))
    flat = FlatParams(model)
    optimizer = FlatAdam(flat, lr=opt.lr)
    criterion = Loss()
    best_val_cost = np.inf
    st_time = time.time()
    history = {"train": [], "test": [], "shares": []}
    score = None
    if opt.seg_score:
        from densefusion_amd.lib.segment_score import SegScore
        score, history["miou"] = SegScore(K, dev), []

    def feed(ds, order, batch_size):
        batches = ds.batches(order, batch_size)
        return train_utils.Prefetcher(batches, range(len(batches)), dev, workers=opt.workers)

    for epoch in range(1, opt.n_epochs):
        model.train()
        costs, train_time = [], 0
        logger = setup_logger("epoch%d" % epoch, os.path.join(opt.log_dir, "epoch_%d_log.txt" % epoch))
        logger.info("Train time {0}".format(_clock(st_time) + ", " + "Training started"))
        if opt.cad_fresh:
            dataset.set_epoch(epoch - 1)
        pixels = torch.zeros(K, dtype=torch.int64, device=dev)
        pf = feed(dataset, dataset.permutation(np.random.RandomState(opt.manualSeed + epoch)), opt.batch_size)
        try:
            for x, target, counts in pf:
                semantic = model.forward_nhwc(x)
                flat.zero_grad()
                semantic_loss = criterion(semantic, target)
                semantic_loss.backward()
                optimizer.step()
                pixels += counts
                costs.append(semantic_loss.item())
                logger.info("Train time {0} Batch {1} CEloss {2}".format(_clock(st_time), train_time, costs[-1]))
                train_time += 1
        finally:
            pf.close()
        torch.save(_plain_state_dict(model), os.path.join(opt.model_save_path, "model_current.pth"))
        logger.info("Train Finish Avg CEloss: {0}".format(sum(costs) / max(train_time, 1)))
        shares = (pixels.double() / pixels.sum().clamp(min=1)).tolist()        # the epoch's one read-back of the counts
        logger.info("Class pixel shares: {0}".format(" ".join("%.4f" % s for s in shares)))
        history["train"].append(costs)
        history["shares"].append(shares)

        model.eval()
        costs = []
        logger = setup_logger("epoch%d_test" % epoch, os.path.join(opt.log_dir, "epoch_%d_test_log.txt" % epoch))
        logger.info("Test time {0}".format(_clock(st_time) + ", " + "Testing started"))
        pf = feed(test_dataset, range(len(test_dataset)), 1)
        if score is not None:
            score.reset()
        try:
            with torch.no_grad():
                for x, target, _ in pf:
                    a = model.forward_nhwc(x)
                    semantic = a[..., :K].permute(0, 3, 1, 2)
                    semantic._nhwc = a                                          # Loss reads the channels-last logits directly
                    costs.append(criterion(semantic, target).item())
                    if score is not None:
                        score.update(a, target)                                 # on the logits the loss just read; nothing comes back
                    logger.info("Test time {0} Batch {1} CEloss {2}".format(_clock(st_time), len(costs), costs[-1]))
        finally:
            pf.close()
        test_all_cost = sum(costs) / max(len(costs), 1)
        logger.info("Test Finish Avg CEloss: {0}".format(test_all_cost))
        history["test"].append(costs)
        if score is not None:
            m = score.summary()                                                 # the test pass's one read-back of the matrix
            logger.info("Test Finish mIoU: {0:.4f} IoU: {1}".format(m["miou"], " ".join("%.4f" % v for v in m["iou"])))
            history["miou"].append(m["miou"])

        if test_all_cost <= best_val_cost:
            best_val_cost = test_all_cost
            torch.save(_plain_state_dict(model), os.path.join(opt.model_save_path, "model_{}_{}.pth".format(epoch, test_all_cost)))
            print("----------->BEST SAVED<-----------")
    return history


def main(argv=None):
    opt = build_parser().parse_args(argv)
    opt.manualSeed = random.randint(1, 10000) if opt.seed is None else opt.seed
    random.seed(opt.manualSeed)
    np.random.seed(opt.manualSeed)
    torch.manual_seed(opt.manualSeed)
    if not torch.cuda.is_available():
        raise SystemExit("train_segnet.py needs a GPU (densefusion_amd has no CPU path)")
    os.makedirs(opt.model_save_path, exist_ok=True)
    os.makedirs(opt.log_dir, exist_ok=True)
    if opt.dataset == "cad_render":
        return train_cad(opt)

    cfg = opt.dataset_config_dir
    dataset = SegDataset(opt.dataset_root, os.path.join(cfg, "train_data_list.txt"), True, opt.train_length)
    dataloader = torch.utils.data.DataLoader(dataset, batch_size=opt.batch_size, shuffle=True, num_workers=opt.workers)
    test_dataset = SegDataset(opt.dataset_root, os.path.join(cfg, "test_data_list.txt"), False, opt.test_length)
    test_dataloader = torch.utils.data.DataLoader(test_dataset, batch_size=1, shuffle=True, num_workers=opt.workers)
    print(len(dataset), len(test_dataset))

    model = SegNet(trainable=True).cuda()
    if opt.resume_model != "":
        model.load_state_dict(torch.load(os.path.join(opt.model_save_path, opt.resume_model), map_location="cuda"))
        for log in os.listdir(opt.log_dir):
            os.remove(os.path.join(opt.log_dir, log))
    flat = FlatParams(model)
    optimizer = FlatAdam(flat, lr=opt.lr)
    criterion = Loss()
    best_val_cost = np.inf
    st_time = time.time()

    for epoch in range(1, opt.n_epochs):
        model.train()
        train_all_cost, train_time = 0.0, 0
        logger = setup_logger("epoch%d" % epoch, os.path.join(opt.log_dir, "epoch_%d_log.txt" % epoch))
        logger.info("Train time {0}".format(_clock(st_time) + ", " + "Training started"))
        for rgb, target in dataloader:
            rgb, target = rgb.cuda(non_blocking=True), target.cuda(non_blocking=True)
            semantic = model(rgb)
            flat.zero_grad()
            semantic_loss = criterion(semantic, target)
            semantic_loss.backward()
            optimizer.step()
            cost = semantic_loss.item()
            train_all_cost += cost
            logger.info("Train time {0} Batch {1} CEloss {2}".format(_clock(st_time), train_time, cost))
            if train_time != 0 and train_time % 1000 == 0:
                torch.save(_plain_state_dict(model), os.path.join(opt.model_save_path, "model_current.pth"))
            train_time += 1
        train_all_cost = train_all_cost / max(train_time, 1)
        logger.info("Train Finish Avg CEloss: {0}".format(train_all_cost))

        model.eval()
        test_all_cost, test_time = 0.0, 0
        logger = setup_logger("epoch%d_test" % epoch, os.path.join(opt.log_dir, "epoch_%d_test_log.txt" % epoch))
        logger.info("Test time {0}".format(_clock(st_time) + ", " + "Testing started"))
        with torch.no_grad():
            for rgb, target in test_dataloader:
                rgb, target = rgb.cuda(non_blocking=True), target.cuda(non_blocking=True)
                semantic_loss = criterion(model(rgb), target)
                test_all_cost += semantic_loss.item()
                test_time += 1
                logger.info("Test time {0} Batch {1} CEloss {2}".format(_clock(st_time), test_time, semantic_loss.item()))
        test_all_cost = test_all_cost / max(test_time, 1)
        logger.info("Test Finish Avg CEloss: {0}".format(test_all_cost))

        if test_all_cost <= best_val_cost:
            best_val_cost = test_all_cost
            torch.save(_plain_state_dict(model), os.path.join(opt.model_save_path, "model_{}_{}.pth".format(epoch, test_all_cost)))
            print("----------->BEST SAVED<-----------")


if __name__ == "__main__":
    main()
