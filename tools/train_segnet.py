"""Train the SegNet mask network (the reference's vanilla_segmentation/train.py) on the HIP training path.

Same flags and loop as the reference: per epoch a training pass over SegDataset(train list, noise on, --train_length frames; the
reference uses 5000) logging ``CEloss`` per batch, ``model_current.pth`` every 1000 batches, a test pass in eval() over
SegDataset(test list, no noise, --test_length frames; reference 1000) and ``model_{epoch}_{cost}.pth`` on a new best test loss.
Checkpoints are plain state dicts in the reference's key layout.  The optimiser is Adam with the reference's defaults, through
FlatAdam over one flat parameter buffer (df_adam_step); --dataset_config_dir locates train_data_list.txt / test_data_list.txt as
tools/train.py does.

    python tools/train_segnet.py --dataset_root YCB_Video_Dataset --dataset_config_dir datasets/ycb/dataset_config
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
