"""The measuring method of the operator target tools (tools/*_target.py), written once.  Every table under
profiles/*_target.md that one of them printed can be compared with the others because all of them measure this way:

Interleaved: REPS rounds of alternating batches of BATCH calls, device events around each batch, median [min..max] of the
per-call time; every call of a batch takes the next of SETS change sets.

The batches are interleaved because that is how this project measures a difference: two versions compared in the same
call, alternating, meet the same clocks, the same neighbours on the device and the same drift, which two runs one after
the other do not.  A tool hands `rounds` its runs -- (key, fn) pairs, fn(i) one call on change set i % SETS -- after it
has checked their results, and prints `fmt` of the times it gets back.

The inputs are written once here as well: `change_sets` draws the changed blocks, `pack` gives a map the library's mask
layout, `device_sets` puts both operand forms on the device, `moving_frames` makes the frames of the chain tables.  Table
headers and row layouts differ per tool and stay there.  Nothing here touches the device when the module is imported."""
import statistics

import numpy as np

try:
    import torch
except ImportError:      # (change_sets, pack, fmt and rounds need numpy alone)
    torch = None

BATCH, SETS = 32, 16


def timed(fn, n):
    """mean device time of fn(i) in us over n back-to-back calls (the caller has warmed fn up)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def rounds(runs, reps, warm=1):
    """{key: [reps times]} of the (key, fn) pairs in `runs`: `warm` warm-up batches per run (one is two passes over the
    change sets), then reps rounds of one timed batch per run, in the order given."""
    for _, fn in runs:
        for _ in range(warm):
            timed(fn, BATCH)
    t = {key: [] for key, _ in runs}
    for _ in range(reps):
        for key, fn in runs:
            t[key].append(timed(fn, BATCH))
    return t


def change_sets(rng, H, W, block, share):
    """SETS bool maps with `share` of the block x block tiles set."""
    by, bx = (H + block - 1) // block, (W + block - 1) // block
    out = []
    for _ in range(SETS):
        tiles = np.zeros(by * bx, dtype=bool)
        tiles[rng.choice(by * bx, size=max(1, round(share * by * bx)), replace=False)] = True
        out.append(np.kron(tiles.reshape(by, bx), np.ones((block, block), dtype=bool))[:H, :W])
    return out


def pack(mask):
    """bool [H, W] -> int64 [H * wpr]: bit x % 64 of word row * wpr + x / 64."""
    H, W = mask.shape
    wpr = (W + 63) // 64
    pad = np.zeros((H, wpr * 64), dtype=bool)
    pad[:, :W] = mask
    return np.packbits(pad.reshape(H, wpr, 64), axis=-1, bitorder='little').reshape(-1).view('<u8').view(np.int64).copy()


def fmt(v):
    return "%.1f [%.1f..%.1f]" % (statistics.median(v), min(v), max(v))


def device_sets(sets):
    """(masks, lists): every change set on the device in the two operand forms, packed mask words and ascending int32
    pixel indexes."""
    masks = [torch.from_numpy(pack(m)).cuda() for m in sets]
    lists = [torch.from_numpy(np.flatnonzero(m.reshape(-1)).astype(np.int32)).cuda() for m in sets]
    return masks, lists


def listed_share(sets):
    """mean share of set pixels over the maps, in percent"""
    return statistics.mean(float(m.mean()) for m in sets) * 100.0


def dtype_name(dtype):
    return "fp32" if dtype == torch.float32 else "fp16"


def moving_frames(base, sets, channels, dtype):
    """Frame i is the base with fresh values on set i: it differs from frame i - 1 on set i and set i - 1."""
    frames = []
    for m in sets:
        f = base.clone()
        f[0][:, torch.from_numpy(m).cuda()] = torch.rand(channels, int(m.sum()), device="cuda").to(dtype)
        frames.append(f)
    return frames
