"""ctypes binding of the spatial-compatibility hypothesis kernels (csrc/sc2.hip; include/roreg_hip.h "v6m"): part of the `roreg_amd.hip`
namespace (hip.py re-exports everything here).  No reference counterpart; tests/_sc2_oracle.py restates the definition in numpy."""
import ctypes
import os

import numpy as np
import torch

from ._abi import _SC2_TASK
from .hip import HipError, _check, _ptr, _stream, lib, upload

__all__ = ['SC2_MAX_M', 'SC2_SEED_TILE', 'SC2_COL_TILE', 'SC2_WORKSPACE_CAP', 'sc2_hypotheses_batch']

SC2_MAX_M = 8192             # == ROREG_SC2_MAX_M: the rank key packs the row index into 13 bits
SC2_SEED_TILE = 64           # == ROREG_SC2_SEED_TILE / ROREG_SC2_COL_TILE: the second-order kernel's tile (tests straddle its edges)
SC2_COL_TILE = 64
# bytes of workspace one launch group may take (the pairs of a call are chunked under it; a single pair above it is a group of its own)
SC2_WORKSPACE_CAP = int(os.environ.get('ROREG_SC2_WORKSPACE_MB', 1024)) << 20

_GUARD = 0xA5                # debug=True: the workspace and the outputs are filled with this byte first, the guards behind them checked after


def _pair_bytes(M, S):
    return M * 48 + M * ((M + 63) // 64) * 8 + M * 4 + S * M * 2 + 5 * 320


def sc2_hypotheses_batch(tasks, tau, max_seeds=1000, K=20, debug=False, workspace_cap=None):
    """tasks: [(keys0 [*,3] f64, keys1 [*,3] f64, matches [M,2] int64)] (device tensors) -> (Trans [sum S,3,4] f64 device, [(offset, S)] per task):
    rows [offset, offset + S) are the task's hypotheses in seed order, S = min(M, max_seeds).  Six launches per group of pairs under the
    workspace cap, no host synchronisation.
    debug=True: a third value, one dict per task of host arrays -- bits uint64 [M, ceil(M/64)], deg int32 [M], seeds int32 [S], N2 uint16 [S,M],
    cons int32 [S,K] (-1 padded), guards_ok (the bytes behind every workspace region and every output were left alone)."""
    from .engine import even_groups
    n = len(tasks)
    tau = float(tau); K = int(K); max_seeds = int(max_seeds)
    if not (3 <= K <= 64):
        raise ValueError(f'sc2_hypotheses_batch: K must lie in 3..64, got {K}')
    if not (tau >= 0.0 and np.isfinite(tau)) or max_seeds < 0:
        raise ValueError('sc2_hypotheses_batch: tau must be finite and >= 0, max_seeds >= 0')
    dev = tasks[0][0].device if n else torch.device('cuda')
    Ms = []
    for k0, k1, m in tasks:
        _ptr(k0, torch.float64); _ptr(k1, torch.float64); _ptr(m, torch.int64)
        if m.dim() != 2 or m.shape[1] != 2 or k0.dim() != 2 or k0.shape[1] != 3 or k1.dim() != 2 or k1.shape[1] != 3:
            raise HipError('sc2_hypotheses_batch: keys must be [*,3] float64 and matches [M,2] int64')
        if int(m.shape[0]) > SC2_MAX_M:
            raise HipError(f'sc2_hypotheses_batch: {int(m.shape[0])} correspondences in a pair, at most {SC2_MAX_M} are supported')
        Ms.append(int(m.shape[0]))
    Ss = [min(M, max_seeds) for M in Ms]
    offsets, o = [], 0
    for S in Ss:
        offsets.append((o, S)); o += S
    total_S = o
    pad = 8 if debug else 0                                       # guard rows behind the outputs
    Trans = torch.empty((total_S + pad, 3, 4), dtype=torch.float64, device=dev)
    seeds = torch.empty(total_S + pad * 16, dtype=torch.int32, device=dev)
    cons = torch.empty((total_S + pad, K), dtype=torch.int32, device=dev) if debug else None
    if debug:
        for t in (Trans, seeds, cons):
            t.view(torch.uint8).fill_(_GUARD)
    dbg = [None] * n
    guards_ok = True
    cap = SC2_WORKSPACE_CAP if workspace_cap is None else int(workspace_cap)
    for i, j in even_groups([_pair_bytes(M, S) for M, S in zip(Ms, Ss)], cap):
        table = np.zeros(j - i, _SC2_TASK)
        koff = boff = noff = 0
        for q in range(i, j):
            k0, k1, m = tasks[q]
            M, S = Ms[q], Ss[q]
            table[q - i] = (k0.data_ptr(), k1.data_ptr(), m.data_ptr() if M else 0, M, S, koff, boff, offsets[q][0], noff)
            koff += M; boff += M * ((M + 63) // 64); noff += S * M
        max_M, max_S = max(Ms[i:j]), max(Ss[i:j])
        if max_M == 0:
            for q in range(i, j):
                dbg[q] = dict(bits=np.zeros((0, 0), np.uint64), deg=np.zeros(0, np.int32), seeds=np.zeros(0, np.int32), N2=np.zeros((0, 0), np.uint16),
                              cons=np.zeros((0, K), np.int32))
            continue
        offs = (ctypes.c_size_t * 5)()
        ws_n = lib().roreg_sc2_workspace(koff, boff, noff, ctypes.cast(offs, ctypes.c_void_p))
        ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
        if debug:
            ws.fill_(_GUARD)
        tdev = upload(table.view(np.uint8).reshape(j - i, _SC2_TASK.itemsize))
        _check(lib().roreg_sc2_hypotheses_batch(_ptr(tdev), j - i, koff, boff, noff, max_M, max_S, tau, K, _ptr(Trans), _ptr(seeds), _ptr(cons),
                                                _ptr(ws), ws_n, _stream()), 'roreg_sc2_hypotheses_batch')
        if debug:
            w = ws.cpu().numpy()
            ends = [offs[0] + koff * 24, offs[1] + koff * 24, offs[2] + boff * 8, offs[3] + koff * 4, offs[4] + noff * 2]
            nexts = [offs[1], offs[2], offs[3], offs[4], ws_n]
            guards_ok = guards_ok and all(e + 64 <= nx and (w[e:nx] == _GUARD).all() for e, nx in zip(ends, nexts))
            bits = w[offs[2]:offs[2] + boff * 8].view(np.uint64); deg = w[offs[3]:offs[3] + koff * 4].view(np.int32)
            N2 = w[offs[4]:offs[4] + noff * 2].view(np.uint16)
            seeds_h = seeds.cpu().numpy(); cons_h = cons.cpu().numpy()
            for q in range(i, j):
                M, S = Ms[q], Ss[q]
                W = (M + 63) // 64
                r = table[q - i]
                dbg[q] = dict(bits=bits[r['boff']:r['boff'] + M * W].reshape(M, W).copy(), deg=deg[r['koff']:r['koff'] + M].copy(),
                              seeds=seeds_h[offsets[q][0]:offsets[q][0] + S].copy(), N2=N2[r['noff']:r['noff'] + S * M].reshape(S, M).copy(),
                              cons=cons_h[offsets[q][0]:offsets[q][0] + S].copy())
        del ws
    if not debug:
        return Trans, offsets
    g = int(_GUARD)
    guards_ok = bool(guards_ok and (Trans[total_S:].view(torch.uint8) == g).all() and (seeds[total_S:].view(torch.uint8) == g).all()
                     and (cons[total_S:].view(torch.uint8) == g).all())
    for d in dbg:
        d['guards_ok'] = guards_ok
    return Trans[:total_S], offsets, dbg
