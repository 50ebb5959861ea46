"""Inputs and references for the tests that push a batch entry across the place where it cuts a long batch (tests/test_batch_cuts_cpu.py, tests/test_batch_cuts_gpu.py).

Two ways to make tens of thousands of frames whose expected result costs little:
  periodic(frames_P, n)   frame i is frames_P[i % P] with P = 251, a prime: the oracle is computed for P frames, and a wrong first-frame offset of a later launch, a
                          frame index that restarts with each launch or a skipped frame shows, because no cut of the library is a multiple of 251 (65535 % 251 = 24)
  all4x4(n)               frame i has bit k of i % 65536 as its pixel k (times 255): 65536 frames are every binary 4 x 4 image, each a different problem for the
                          labelling and the distance transform; label4x4 / dist4x4 below answer all of them at once in numpy and are held against the per-image
                          restatements (ccl_restate.label, disttransform_restate.distanceTransform) by the CPU test
and the parsing of what mi355cv_lastKernel says about the cut."""
import re

import numpy as np

import ccl_restate as C
import disttransform_restate as D

P = 251


def periodic(frames_P, n):
    frames_P = np.asarray(frames_P)
    assert frames_P.shape[0] == P
    return np.ascontiguousarray(frames_P[np.arange(n) % P])


def same_periodic(got, want_P):
    """every frame of got equals want_P[i % P] (one comparison); -> (ok, the first wrong frame or None)"""
    got, want_P = np.asarray(got), np.asarray(want_P)
    if got.shape[1:] != want_P.shape[1:] or got.dtype != want_P.dtype:
        return False, None
    bad = (got.view(np.uint8).reshape(got.shape[0], -1) != want_P.view(np.uint8).reshape(P, -1)[np.arange(got.shape[0]) % P]).any(axis=1)
    return not bad.any(), (int(np.flatnonzero(bad)[0]) if bad.any() else None)


def all4x4(n):
    i = (np.arange(n, dtype=np.int64) % 65536)[:, None]
    return ((((i >> np.arange(16)[None, :]) & 1) * 255).astype(np.uint8)).reshape(n, 4, 4)


# ---- the 16 pixels of a 4 x 4 image and their neighbours
_Y, _X = np.divmod(np.arange(16), 4)


def _neighbours(connectivity):
    """[16, k] pixel indices of the neighbours, the pixel itself where the image ends"""
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    nb = np.empty((16, len(steps)), np.int64)
    for j, (dy, dx) in enumerate(steps):
        y, x = _Y + dy, _X + dx
        ok = (y >= 0) & (y < 4) & (x >= 0) & (x < 4)
        nb[:, j] = np.where(ok, y * 4 + x, np.arange(16))
    return nb


def label4x4(frames, connectivity=8, order=C.PIXEL):
    """-> (n int32 [N], labels int32 [N, 4, 4]) by the rule of ccl_restate.label: every foreground pixel takes the smallest key of its component by propagating
    minima to the neighbours until nothing changes (16 rounds reach across any path in 16 pixels), components are numbered 1, 2, ... by (smallest key, smallest
    pixel index); the key is the pixel index y * 4 + x (PIXEL) or the 2 x 2 block index (y >> 1) * 2 + (x >> 1) (BLOCK)"""
    fg = np.asarray(frames).reshape(-1, 16) != 0
    big = np.int32(1 << 20)
    pkey = np.arange(16, dtype=np.int32)
    key = pkey if order == C.PIXEL else ((_Y >> 1) * 2 + (_X >> 1)).astype(np.int32)
    nb = _neighbours(connectivity)
    pmin = np.where(fg, pkey[None, :], big)                       # the smallest pixel index and the smallest key of a component need not belong to the
    kmin = np.where(fg, key[None, :], big)                        # same pixel (BLOCK): the two minima are propagated separately
    for m in (pmin, kmin):
        for _ in range(16):
            around = m[:, nb].min(axis=2)                          # [N, 16]: the smallest value among the neighbours (background holds `big`)
            new = np.where(fg, np.minimum(m, around), big)
            if np.array_equal(new, m):
                break
            m[...] = new
    rank = kmin * 16 + pmin                                        # one number per component, ordered as the labels are
    root = fg & (pmin == pkey[None, :])                            # the pixel with the smallest index of each component
    rootrank = np.where(root, rank, big)
    labels = np.where(fg, 1 + (rootrank[:, None, :] < rank[:, :, None]).sum(axis=2), 0).astype(np.int32)
    return (root.sum(axis=1) + 1).astype(np.int32), labels.reshape(-1, 4, 4)


def dist4x4(frames, metric, dtype=np.float32):
    """the served distance transform of every frame: the minimum over the 16 possible sites, brute force; a frame without a zero pixel gets D.NO_SITE_*"""
    site = np.asarray(frames).reshape(-1, 16) == 0
    dy, dx = np.abs(_Y[:, None] - _Y[None, :]), np.abs(_X[:, None] - _X[None, :])       # [pixel, site]
    table = dy * dy + dx * dx if metric == D.DIST_L2 else dy + dx if metric == D.DIST_L1 else np.maximum(dy, dx)
    far = np.int64(1 << 20)
    d = np.full(site.shape, far, np.int64)
    for s in range(16):
        np.minimum(d, np.where(site[:, s:s + 1], table[None, :, s], far), out=d)
    none = d == far
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        assert metric == D.DIST_L1
        out = np.where(none, D.NO_SITE_8U, np.minimum(d, 255)).astype(np.uint8)
    else:
        val = np.sqrt(d.astype(np.float64)).astype(np.float32) if metric == D.DIST_L2 else d.astype(np.float32)
        out = np.where(none, D.NO_SITE_32F, val).astype(np.float32)
    return out.reshape(-1, 4, 4)


# ---- what mi355cv_lastKernel says about the cut
def cut_of(note, nframes):
    """-> (crossed, text): whether the note proves that the batch of nframes frames took more than one launch / group"""
    m = re.search(r"(\d+) launch\(es\) of <= (\d+) frames", note)
    if m:
        return int(m.group(1)) > 1 and int(m.group(2)) < nframes, m.group(0)
    m = re.search(r"in groups of (\d+)", note) or re.search(r"frames=(\d+)/launch", note)
    if m:
        return int(m.group(1)) < nframes, m.group(0)
    m = re.search(r"(\d+) launch\(es\)", note)
    if m:
        return int(m.group(1)) > 1, m.group(0)
    return False, "(the note names no launch count or group)"
