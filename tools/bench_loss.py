"""The library's losses on caller-owned predictions against their restatement in torch ops (DESIGN.md "Native losses on caller predictions"):

    python tools/bench_loss.py [--steps K] [--warmup W] [--reps R] [--out-dir profiles] [--note-file FILE ...]

For RelativeL2 and L1, half and float predictions, at n = 2^18 with dims 3 compact, dims 3 in rows of stride 16 (a slice of a module's
padded output) and dims 16, and at 2^21 x 16:
  (a) forward_backward   tcnn.losses.Loss: loss = L(prediction, target); loss.backward()      -- 3 launches: sum, its second stage, gradient
  (b) evaluate           tcnn.losses.Loss.evaluate: loss and gradient in one pass               -- 2 launches
  (c) torch_eager        the same loss in torch ops (float32 arithmetic, mean), forward + backward
Times are device events on the stream around K calls, after W warm-up calls of every arm at every shape; R >= 50 repetitions with the
arms alternating repetition by repetition; median (min - max).  Bytes are what the kernels have to move, computed from the shapes: the
prediction as it is loaded (a padded row: its 16-byte vectors that start at a value), the target, the gradient written; the implied bandwidth is
those bytes over the median time -- far below HBM's at 2^18 x 3, where the launches are the cost.
Writes <out-dir>/native_loss_bench.txt and .json; --note-file appends text (the bench.py lines of this commit and its parent)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))
import torch  # noqa: E402

import tinycudann as tcnn  # noqa: E402

SHAPES = [("2^18 x 3 compact", 1 << 18, 3, 3), ("2^18 x 3 in stride 16", 1 << 18, 3, 16), ("2^18 x 16", 1 << 18, 16, 16), ("2^21 x 16", 1 << 21, 16, 16)]


def eager(name, prediction, target):
    """the reference's loss (losses/relative_l2.h, l1.h) in torch ops: the normaliser of RelativeL2 is not differentiated"""
    p = prediction.float()
    if name == "L1":
        return (p - target).abs().mean()
    return ((p - target).square() / (p.detach().square() + 0.01)).mean()


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--note-file", action="append", default=[])
    a = ap.parse_args()
    if a.reps < 50:
        raise SystemExit("bench_loss.py: the median is taken over at least 50 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss.py needs a GPU")
    torch.manual_seed(0)
    rows, lines = [], []
    header = f"{a.reps} repetitions x {a.steps} calls after {a.warmup} warm-up calls, device events; median (min - max) us; torch {torch.__version__}"
    print(header, flush=True)
    lines.append(header)
    for name in ("RelativeL2", "L1"):
        loss_fn = tcnn.losses.Loss(name)
        for dtype in (torch.half, torch.float32):
            for label, n, dims, stride in SHAPES:
                storage = (torch.rand(n, stride, device="cuda") * 1.95 + 0.05).to(dtype)
                target = torch.rand(n, dims, device="cuda") * 1.95 + 0.05
                leaf = storage.clone().requires_grad_()
                plain = storage[:, :dims]

                def view(leaf, dims=dims, stride=stride):  # (compact rows: the leaf itself, no slice node in the graph)
                    return leaf if stride == dims else leaf[:, :dims]

                def forward_backward(leaf=leaf, view=view, target=target, loss_fn=loss_fn):
                    leaf.grad = None
                    loss_fn(view(leaf), target).backward()

                def evaluate(plain=plain, target=target, loss_fn=loss_fn):
                    loss_fn.evaluate(plain, target)

                def torch_eager(leaf=leaf, view=view, target=target, name=name):
                    leaf.grad = None
                    eager(name, view(leaf), target).backward()

                arms = {"forward_backward": forward_backward, "evaluate": evaluate, "torch_eager": torch_eager}
                for fn in arms.values():
                    for _ in range(a.warmup):
                        fn()
                torch.cuda.synchronize()
                times = {k: [] for k in arms}
                for _ in range(a.reps):  # alternating: every arm sees the same clocks and the same neighbours
                    for k, fn in arms.items():
                        times[k].append(timed(fn, a.steps) * 1e3)
                elem = storage.element_size()
                # prediction as loaded (compact: every value once; padded rows: the 16-byte vectors that start at a value) + target
                row_bytes = dims * elem if stride == dims else -(-dims * elem // 16) * 16
                read = n * row_bytes + n * dims * 4
                grad = n * dims * elem
                bytes_moved = {"forward_backward": 2 * read + grad, "evaluate": read + grad}
                row = {"loss": name, "dtype": str(dtype).replace("torch.", ""), "shape": label, "n": n, "dims": dims, "stride": stride, "bytes": bytes_moved}
                for k, t in times.items():
                    row[k] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
                    if k in bytes_moved:
                        row[k]["implied_GB_per_s"] = bytes_moved[k] / (row[k]["median_us"] * 1e-6) / 1e9
                row["faster_than_eager"] = all(row[k]["median_us"] < row["torch_eager"]["median_us"] for k in bytes_moved)
                rows.append(row)
                text = f"{name:10s} {row['dtype']:7s} {label:22s}"
                for k in arms:
                    r = row[k]
                    text += f" | {k} {r['median_us']:8.1f} ({r['min_us']:.1f} - {r['max_us']:.1f})"
                    if k in bytes_moved:
                        text += f" {bytes_moved[k] / 1e6:6.1f} MB {r['implied_GB_per_s']:7.1f} GB/s"
                text += f" | eager/(a) {row['torch_eager']['median_us'] / row['forward_backward']['median_us']:.2f} eager/(b) {row['torch_eager']['median_us'] / row['evaluate']['median_us']:.2f}"
                text += " | ok" if row["faster_than_eager"] else " | NOT FASTER"
                print(text, flush=True)
                lines.append(text)
                del storage, target, leaf, plain
    ok = all(r["faster_than_eager"] for r in rows)
    verdict = f"(a) and (b) faster than (c) in every row: {ok}"
    print(verdict, flush=True)
    lines.append(verdict)
    notes = []
    for path in a.note_file:
        with open(path) as f:
            notes.append(f.read().rstrip("\n"))
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "native_loss_bench.txt"), "w") as f:
        f.write("\n".join(lines + notes) + "\n")
    with open(os.path.join(a.out_dir, "native_loss_bench.json"), "w") as f:
        json.dump({"steps": a.steps, "warmup": a.warmup, "reps": a.reps, "torch": torch.__version__, "rows": rows, "all_faster_than_eager": ok, "notes": notes}, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
