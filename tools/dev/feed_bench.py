"""Dev tool: does the trainer's data feed keep up?  Frames/s of the native PoseNet training loop on a fabricated LineMOD tree (PNG
decoding, gt.yml, .ply models: densefusion_amd.datasets.linemod) fed through train_utils.Prefetcher with 0 / 4 / 8 worker threads
and with 8 / 12 worker processes, against the same loop over frames that already sit in device memory.  --add_noise builds the dataset
the way tools/train.py does (colour jitter + translation noise); --jitter host|device says where the jitter's pixel work runs.
--compare times the three feeds of a training run side by side in ONE process -- add_noise off, add_noise with the jitter on the host, add_noise
with the jitter on the device -- through worker processes, taking turns over several rounds (a shared host: single passes scatter widely),
and prints each one's median and range.
usage: feed_bench.py TREE_ROOT [--add_noise] [--jitter host|device] [--frames N] [--workers 0,4,8] [--processes 8,12] [--compare --rounds R]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from densefusion_amd import synth, train_utils
from densefusion_amd.native_train import Lanes, NativeTrainer


def _training_loop(dev, sym, lanes_n):
    """The native PoseNet loop the feeds are timed under: windows of 8 frames on `lanes_n` lanes, one optimizer step each."""
    K, N = 13, 500
    tr = NativeTrainer("posenet", N, K, dev)
    tr.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(synth.posenet_spec(K), 21).items()})
    opt = train_utils.FlatAdam(tr, lr=1e-4)
    lanes = Lanes(tr, lanes_n)

    def loop(items):
        window, n = [], 0
        for it in items:
            if it[0].dim() == 1:
                continue
            window.append(it)
            if len(window) == 8:
                jobs = [(lambda lane, f=f: lane.step_posenet(f[2][None], f[0][None], f[1], f[5], f[3][None], f[4][None],
                                                              [train_utils.host_index(f[5]) in sym], 0.015)) for f in window]
                lanes.run(jobs)
                opt.step(grad_scale=1.0 / 8); tr.zero_grad()
                n += len(window)
                window = []
        torch.cuda.synchronize()
        return n

    return loop, lanes


def run(root, workers_list=(0, 4, 8), frames=96, lanes_n=4, out=print, processes_list=(8, 12), add_noise=False, jitter="host"):
    from densefusion_amd.datasets.linemod.dataset import PoseDataset
    dev = torch.device("cuda")
    ds = PoseDataset("train", 500, add_noise, root, 0.03 if add_noise else 0.0, False, jitter=jitter)
    loop, lanes = _training_loop(dev, ds.get_sym_list(), lanes_n)
    order = [i % len(ds) for i in range(frames)]
    resident = [ds[i] for i in order]
    loop(resident[:16])                        # warm-up: workspaces, weight copies
    t0 = time.perf_counter(); n = loop(resident); base = n / (time.perf_counter() - t0)
    res = {"add_noise": bool(add_noise), "jitter": jitter if add_noise else None, "frames": frames, "resident_frames_per_s": round(base, 1)}
    for w in workers_list:
        t0 = time.perf_counter()
        n = loop(train_utils.Prefetcher(ds, order, dev, workers=w))
        res[f"workers_{w}_frames_per_s"] = round(n / (time.perf_counter() - t0), 1)
    for w in processes_list:
        pf = train_utils.Prefetcher(ds, order, dev, workers=0, processes=w)
        loop(pf.set_order(order[:16]))           # the worker processes start (imports) outside the timed pass, as in a long run
        t0 = time.perf_counter()
        n = loop(pf.set_order(order))
        res[f"processes_{w}_frames_per_s"] = round(n / (time.perf_counter() - t0), 1)
        pf.close()
    lanes.close()
    out(res)
    return res


def compare(root, frames=640, processes=8, rounds=5, lanes_n=4, out=print):
    import statistics
    from densefusion_amd.datasets.linemod.dataset import PoseDataset
    dev = torch.device("cuda")
    feeds = {"add_noise_off": PoseDataset("train", 500, False, root, 0.0, False),
             "add_noise_host_jitter": PoseDataset("train", 500, True, root, 0.03, False, jitter="host"),
             "add_noise_device_jitter": PoseDataset("train", 500, True, root, 0.03, False, jitter="device")}
    loop, lanes = _training_loop(dev, feeds["add_noise_off"].get_sym_list(), lanes_n)
    order = [i % len(feeds["add_noise_off"]) for i in range(frames)]
    pfs = {k: train_utils.Prefetcher(ds, order, dev, workers=0, processes=processes) for k, ds in feeds.items()}
    for pf in pfs.values():
        loop(pf.set_order(order[:32]))           # the worker processes start (imports) outside the timed passes, as in a long run
    rates = {k: [] for k in pfs}
    for _ in range(rounds):
        for k, pf in pfs.items():
            t0 = time.perf_counter()
            n = loop(pf.set_order(order))
            rates[k].append(n / (time.perf_counter() - t0))
    for pf in pfs.values():
        pf.close()
    lanes.close()
    res = {"frames": frames, "processes": processes, "rounds": rounds, "host_cpus": len(os.sched_getaffinity(0)), "cpu_count": os.cpu_count()}
    for k, v in rates.items():
        res[k] = {"median_frames_per_s": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
    out(res)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("root")
    ap.add_argument("--add_noise", action="store_true")
    ap.add_argument("--jitter", default="host", choices=["host", "device"])
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--workers", default="0,4,8", help="thread counts to time, comma-separated (empty: none)")
    ap.add_argument("--processes", default="8,12", help="process counts to time, comma-separated (empty: none)")
    ap.add_argument("--compare", action="store_true", help="the three feeds side by side (the first of --processes), --rounds passes each")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    ints = lambda s: tuple(int(v) for v in s.split(",") if v)
    if a.compare:
        compare(a.root, frames=a.frames, processes=ints(a.processes)[0], rounds=a.rounds)
        sys.exit(0)
    run(a.root, workers_list=ints(a.workers), frames=a.frames, processes_list=ints(a.processes), add_noise=a.add_noise, jitter=a.jitter)
