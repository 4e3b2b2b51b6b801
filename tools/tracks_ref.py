"""numpy union-find restatement of the device track builder (roma_amd/csrc/tracks.hip, roma_amd.build_tracks): the oracle of
tests/test_gpu_views.py, itself pinned by a breadth-first restatement in tests/test_cpu_views.py.  One problem at a time.

  nodes    keypoint i of view v is node v K + i
  edges    row (i, j) of pair p, p's first match_counts[p] rows only, joins (pair_views[p][0], i) to (pair_views[p][1], j); a row
           with an index outside [0, num_kpts[view]) on either side is ignored and counted
  tracks   a connected component with at least min_views nodes and no view twice; a component with two keypoints of one view
           is dropped whole; numbered in ascending order of the smallest node id
"""
from __future__ import annotations

import numpy as np


def build(inds, pair_views, V, K, match_counts=None, num_kpts=None, x=None, max_tracks=None, min_views=2):
    """inds [P, M, 2] int, pair_views [P, 2], match_counts [P] or None, num_kpts [V] or None, x [V, K, 2] float32 or None.  Returns a
    dict: tracks [V, T] int32, kpts [V, T, 2] float32 (None without x), count, total, info = (rows used, rows ignored,
    components of >= 2 nodes, components dropped)."""
    inds = np.asarray(inds).reshape(len(pair_views), -1, 2)
    P, M = inds.shape[:2]
    T = K if max_tracks is None else int(max_tracks)
    nk = np.full(V, K) if num_kpts is None else np.clip(np.asarray(num_kpts), 0, K)
    parent = np.arange(V * K)

    def find(u):
        r = u
        while parent[r] != r:
            r = parent[r]
        while parent[u] != r:
            parent[u], u = r, parent[u]
        return r

    used = ignored = 0
    for p in range(P):
        a, b = int(pair_views[p][0]), int(pair_views[p][1])
        mc = M if match_counts is None else min(max(int(match_counts[p]), 0), M)
        for i, j in inds[p, :mc]:
            if not (0 <= i < nk[a] and 0 <= j < nk[b]):
                ignored += 1
                continue
            used += 1
            ru, rv = find(a * K + int(i)), find(b * K + int(j))
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)  # the root is the smallest id of its component
    members = {}
    for v in range(V):
        for i in range(int(nk[v])):
            members.setdefault(find(v * K + i), []).append((v, i))
    comps = dropped = total = 0
    tracks = np.full((V, T), -1, dtype=np.int32)
    kpts = None if x is None else np.full((V, T, 2), np.nan, dtype=np.float32)
    for root in sorted(members):
        mem = members[root]
        if len(mem) < 2:
            continue
        comps += 1
        views = [v for v, _ in mem]
        if len(set(views)) != len(views):
            dropped += 1
            continue
        if len(mem) < min_views:
            continue
        if total < T:
            for v, i in mem:
                tracks[v, total] = i
                if x is not None:
                    kpts[v, total] = x[v, i]
        total += 1
    return dict(tracks=tracks, kpts=kpts, count=min(total, T), total=total, info=(used, ignored, comps, dropped))
