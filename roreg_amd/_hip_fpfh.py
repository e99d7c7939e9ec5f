"""ctypes bindings of the FPFH kernels (csrc/fpfh.hip; include/roreg_hip.h "v6n") and of their matcher (csrc/fpfh_match.hip; "v6o"): part of
the `roreg_amd.hip` namespace (hip.py re-exports everything here).  No reference counterpart; tests/_fpfh_oracle.py restates the descriptor's
definition in numpy, the matcher's is hip.nn_search + hip.mutual_matches.  Every table is in the cloud's ORIGINAL row order; `grid` is the
cloud's hip.IcpGrid (built for any radius: one built for the FPFH radius walks the fewest cells)."""
import ctypes
import os

import numpy as np
import torch

from ._abi import _FPFH_MATCH_DEBUG, _FPFH_MATCH_TASK
from .hip import HipError, _check, _ptr, _stream, lib, upload

__all__ = ['FPFH_WIDTH', 'fpfh_orient', 'fpfh_spfh', 'fpfh_features', 'FPFH_MATCH_TILE', 'FPFH_MATCH_MAX_ROWS', 'FPFH_MATCH_DEBUG_MAX',
           'FPFH_MATCH_WORKSPACE_CAP', 'FPFH_MATCH_C_DELTA', 'FPFH_MATCH_C_COLLAPSE', 'FPFH_MATCH_MARGIN_MULT', 'fpfh_match_delta', 'fpfh_match_margin',
           'fpfh_match', 'fpfh_match_batch', 'fpfh_match_pass_times']

FPFH_WIDTH = 33                        # csrc/fpfh_math.h WIDTH: 11 bins of each of the three pair features


def _radius(radius, what):
    r = float(radius)
    if not (r > 0.0 and np.isfinite(r)):
        raise HipError(f'{what}: radius must be positive and finite')
    return r


def _normal_table(grid, t, what):
    _ptr(t, torch.float64)
    if tuple(t.shape) != (grid.n, 4) or (grid.n and t.data_ptr() % 32):
        raise HipError(f'{what}: the normal table must be [n,4] float64, 32-byte aligned')


def fpfh_orient(grid, normals, viewpoint):
    """normals f64 [n,4] (hip.icp_normals' table) -> the same table with every valid normal pointing to the side of `viewpoint` (three
    numbers on the host): a row is negated iff n . (viewpoint - x) < 0; a zero row stays zero, column 3 is copied."""
    _normal_table(grid, normals, 'fpfh_orient')
    c = np.ascontiguousarray(np.asarray(viewpoint, np.float64).reshape(-1))
    if c.shape != (3,) or not np.isfinite(c).all():
        raise HipError('fpfh_orient: the viewpoint must be three finite numbers')
    out = torch.empty((grid.n, 4), dtype=torch.float64, device=grid.buf.device)
    if grid.n:
        _check(lib().roreg_fpfh_orient(_ptr(grid.buf), grid.n, _ptr(normals), c.ctypes.data, _ptr(out), _stream()), 'roreg_fpfh_orient')
    return out


def fpfh_spfh(grid, oriented, radius):
    """oriented f64 [n,4] (fpfh_orient) -> (counts int32 [n,33], m int32 [n]): the bins of the pair features of every neighbour within
    `radius` that has a valid normal, and the number of such pairs.  Integers: the same bytes from any grid of the cloud."""
    r = _radius(radius, 'fpfh_spfh')
    _normal_table(grid, oriented, 'fpfh_spfh')
    dev = grid.buf.device
    counts = torch.empty((grid.n, FPFH_WIDTH), dtype=torch.int32, device=dev)
    m = torch.empty(grid.n, dtype=torch.int32, device=dev)
    if grid.n:
        ws_n = lib().roreg_fpfh_spfh_workspace(grid.n)
        ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
        _check(lib().roreg_fpfh_spfh(_ptr(grid.buf), grid.n, _ptr(oriented), r, _ptr(counts), _ptr(m), _ptr(ws), ws_n, _stream()), 'roreg_fpfh_spfh')
    return counts, m


def fpfh_features(grid, counts, m, radius):
    """counts int32 [n,33], m int32 [n] (fpfh_spfh) -> (features f32 [n,33], valid uint8 [n]): every point's own histogram plus the
    1 / d2-weighted histograms of its neighbours within `radius`, each third normalised to 100 + 100.  valid = m > 0; an invalid row is zero."""
    r = _radius(radius, 'fpfh_features')
    _ptr(counts, torch.int32); _ptr(m, torch.int32)
    if tuple(counts.shape) != (grid.n, FPFH_WIDTH) or tuple(m.shape) != (grid.n,):
        raise HipError('fpfh_features: counts must be [n,33] int32 and m [n] int32')
    dev = grid.buf.device
    out = torch.empty((grid.n, FPFH_WIDTH), dtype=torch.float32, device=dev)
    valid = torch.empty(grid.n, dtype=torch.uint8, device=dev)
    if grid.n:
        ws_n = lib().roreg_fpfh_features_workspace(grid.n)
        ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
        _check(lib().roreg_fpfh_features(_ptr(grid.buf), grid.n, _ptr(counts), _ptr(m), r, _ptr(out), _ptr(valid), _ptr(ws), ws_n, _stream()),
               'roreg_fpfh_features')
    return out, valid


# ---- v6o: the matcher (csrc/fpfh_match.hip) ---------------------------------------------------------------------------
FPFH_MATCH_TILE = 128                  # == ROREG_FPFH_MATCH_TILE: edge of a tile of the distance matrix (tests straddle it)
FPFH_MATCH_MAX_ROWS = 1 << 20          # == ROREG_FPFH_MATCH_MAX_ROWS: rows per side
FPFH_MATCH_DEBUG_MAX = 512             # == ROREG_FPFH_MATCH_DEBUG_MAX: a task with both sides at most this long fills its debug arrays
# bytes of workspace one launch group may take (the tasks of a call are chunked under it; a single task above it is a group of its own)
FPFH_MATCH_WORKSPACE_CAP = int(os.environ.get('ROREG_FPFH_MATCH_WORKSPACE_MB', 1024)) << 20
# The error bound of the approximate squared distance and the candidate margin, as csrc/fpfh_match.hip derives them (u = 2^-24):
#   |a(i,j) - x(i,j)| <= delta(i,j) = C_DELTA (N_i + N_j),   N = squared norm over all 33 channels, x = sum_f (s_f - t_f)^2 in real arithmetic
#   margin_i = MARGIN_MULT (2 Delta_i + C_COLLAPSE (max(amin_i, 0) + Delta_i + 1e-7)),   Delta_i = C_DELTA (N_i + max_j N_j)
FPFH_MATCH_C_DELTA = 8 * 2.0 ** -24 + (96 * 2.0 ** -23 + 3.01 * 2.0 ** -22 + 2.0 ** -34)
FPFH_MATCH_C_COLLAPSE = 80 * 2.0 ** -24
FPFH_MATCH_MARGIN_MULT = 2.0
_ROW_BYTES = 36 * 4 + 4 + 4 + 8        # workspace per padded row: the gathered row, its norm, its minimum key, its packed key
_GUARD = 0xA5                          # debug=True: the workspace and the outputs are filled with this byte first, the guards behind them checked after


def fpfh_match_delta(n0, n1):
    """The bound on |a - x| of one entry from the two rows' squared norms (numbers or arrays)."""
    return FPFH_MATCH_C_DELTA * (n0 + n1)


def fpfh_match_margin(amin, n, max_other):
    """The candidate margin of a row (column): amin its approximate minimum, n its squared norm, max_other the other side's greatest."""
    delta = FPFH_MATCH_C_DELTA * (n + max_other)
    return FPFH_MATCH_MARGIN_MULT * (2.0 * delta + FPFH_MATCH_C_COLLAPSE * (np.maximum(amin, 0.0) + delta + 1e-7))


def _pad(m):
    return -(-m // FPFH_MATCH_TILE) * FPFH_MATCH_TILE


def _match_task(task):
    desc0, desc1, rows0, rows1 = (tuple(task) + (None, None))[:4]
    for d in (desc0, desc1):
        _ptr(d, torch.float32)
        if d.dim() != 2 or int(d.shape[1]) != FPFH_WIDTH:
            raise HipError(f'fpfh_match: descriptors must be [*,{FPFH_WIDTH}] float32, got {tuple(d.shape)}')
    ms = []
    for d, r in ((desc0, rows0), (desc1, rows1)):
        if r is not None:
            _ptr(r, torch.int64)
            if r.dim() != 1:
                raise HipError('fpfh_match: a row list must be a 1-d int64 tensor')
        m = int(d.shape[0]) if r is None else int(r.shape[0])
        if m > FPFH_MATCH_MAX_ROWS:
            raise HipError(f'fpfh_match: {m} rows on a side, at most {FPFH_MATCH_MAX_ROWS} are supported')
        ms.append(m)
    return desc0, desc1, rows0, rows1, ms[0], ms[1]


def fpfh_match_batch(tasks, debug=False, workspace_cap=None):
    """tasks: [(desc0 [*,33] f32, desc1 [*,33] f32, rows0, rows1)] (device tensors; the row lists int64 or None = every row) ->
    [(matches int64 [min(m0,m1),2], count int32 [1], nn01 int64 [m0], dist01 f32 [m0], nn10 int64 [m1])] per task, device tensors: bit for
    bit hip.nn_search (F = 33, both directions) and hip.mutual_matches; rows [0, count) of matches are valid, in increasing row of side 0.
    PRECONDITION: every selected row is finite (hip.fpfh_features writes nothing else); rows that are not selected are never read.
    Five launches per group of tasks under the workspace cap, no host synchronisation.  A task with an empty side: empty tensors, count 0,
    and it takes part in no launch.
    debug=True: a sixth value per task, a dict of host arrays: guards_ok (the bytes behind every workspace region and every output were left
    alone), and for a task with both sides <= FPFH_MATCH_DEBUG_MAX: a f32 [m0,m1] the approximate squared distances, amin0 [m0] / amin1 [m1]
    their row / column minima as pass A found them, cnt0 [m0] / cnt1 [m1] the candidates of every row / column."""
    from .engine import even_groups
    parsed = [_match_task(t) for t in tasks]
    n = len(parsed)
    dev = parsed[0][0].device if n else torch.device('cuda')
    out = [None] * n
    live = []
    for q, (d0, d1, r0, r1, m0, m1) in enumerate(parsed):
        if m0 == 0 or m1 == 0:
            out[q] = (torch.zeros((0, 2), dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                      torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.float32, device=dev),
                      torch.zeros(0, dtype=torch.int64, device=dev)) + ((dict(guards_ok=True),) if debug else ())
        else:
            live.append(q)
    cap = FPFH_MATCH_WORKSPACE_CAP if workspace_cap is None else int(workspace_cap)
    guards_ok, dicts = True, []
    for i, j in even_groups([(_pad(parsed[q][4]) + _pad(parsed[q][5])) * _ROW_BYTES for q in live], cap):
        group = live[i:j]
        table = np.zeros(len(group), _FPFH_MATCH_TASK)
        rows = o0 = o1 = om = 0
        for k, q in enumerate(group):
            d0, d1, r0, r1, m0, m1 = parsed[q]
            table[k] = (d0.data_ptr(), d1.data_ptr(), r0.data_ptr() if r0 is not None else 0, r1.data_ptr() if r1 is not None else 0, m0, m1,
                        rows, rows + _pad(m0), o0, o1, om)
            rows += _pad(m0) + _pad(m1); o0 += m0; o1 += m1; om += min(m0, m1)
        pad = 16 if debug else 0                                  # guard elements behind the outputs
        nn01 = torch.empty(o0 + pad, dtype=torch.int64, device=dev)
        dist01 = torch.empty(o0 + pad, dtype=torch.float32, device=dev)
        nn10 = torch.empty(o1 + pad, dtype=torch.int64, device=dev)
        matches = torch.empty((om + pad, 2), dtype=torch.int64, device=dev)
        counts = torch.empty(len(group) + pad, dtype=torch.int32, device=dev)
        offs = (ctypes.c_size_t * 5)()
        ws_n = lib().roreg_fpfh_match_workspace(rows, len(group), ctypes.cast(offs, ctypes.c_void_p))
        ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
        dbg_dev, dbg_arrays = None, {}
        if debug:
            for t in (nn01, dist01, nn10, matches, counts, ws):
                t.view(torch.uint8).fill_(_GUARD)
            dtab = np.zeros(len(group), _FPFH_MATCH_DEBUG)
            for k, q in enumerate(group):
                m0, m1 = parsed[q][4:]
                if m0 <= FPFH_MATCH_DEBUG_MAX and m1 <= FPFH_MATCH_DEBUG_MAX:
                    arr = dict(a=torch.zeros((m0, m1), dtype=torch.float32, device=dev), amin0=torch.zeros(m0, dtype=torch.float32, device=dev),
                               amin1=torch.zeros(m1, dtype=torch.float32, device=dev), cnt0=torch.zeros(m0, dtype=torch.int32, device=dev),
                               cnt1=torch.zeros(m1, dtype=torch.int32, device=dev))
                    dbg_arrays[q] = arr
                    dtab[k] = tuple(arr[name].data_ptr() for name in ('a', 'amin0', 'amin1', 'cnt0', 'cnt1'))
            dbg_dev = upload(dtab.view(np.uint8).reshape(len(group), _FPFH_MATCH_DEBUG.itemsize))
        tdev = upload(table.view(np.uint8).reshape(len(group), _FPFH_MATCH_TASK.itemsize))
        _check(lib().roreg_fpfh_match_batch(_ptr(tdev), len(group), max(parsed[q][4] for q in group), max(parsed[q][5] for q in group), rows,
                                            _ptr(nn01), _ptr(dist01), _ptr(nn10), _ptr(matches), _ptr(counts), _ptr(dbg_dev), _ptr(ws), ws_n,
                                            _stream()), 'roreg_fpfh_match_batch')
        if debug:
            w = ws.cpu().numpy()
            sizes = [rows * 144, rows * 4, rows * 4, rows * 8, len(group) * 8]
            nexts = [offs[1], offs[2], offs[3], offs[4], ws_n]
            guards_ok = guards_ok and all(offs[k] + sizes[k] + 64 <= nexts[k] and (w[offs[k] + sizes[k]:nexts[k]] == _GUARD).all() for k in range(5))
            guards_ok = guards_ok and all(bool((t.reshape(-1)[used:].view(torch.uint8) == _GUARD).all())
                                          for t, used in ((nn01, o0), (dist01, o0), (nn10, o1), (matches, 2 * om), (counts, len(group))))
        for k, q in enumerate(group):
            r = table[k]
            m0, m1 = int(r['m0']), int(r['m1'])
            out[q] = (matches[int(r['om']):int(r['om']) + min(m0, m1)], counts[k:k + 1], nn01[int(r['o0']):int(r['o0']) + m0],
                      dist01[int(r['o0']):int(r['o0']) + m0], nn10[int(r['o1']):int(r['o1']) + m1])
            if debug:
                d = {name: t.cpu().numpy() for name, t in dbg_arrays.get(q, {}).items()}
                dicts.append(d)
                out[q] = out[q] + (d,)
        del ws
    for d in dicts:
        d['guards_ok'] = bool(guards_ok)
    return out


def fpfh_match(desc0, desc1, rows0=None, rows1=None, debug=False):
    """One task of fpfh_match_batch -> (matches, count, nn01, dist01, nn10), and the debug dict when debug=True."""
    return fpfh_match_batch([(desc0, desc1, rows0, rows1)], debug=debug)[0]


def fpfh_match_pass_times():
    """-> (pass A ms, pass B ms) summed over the roreg_fpfh_match_batch calls since hip.profile_enable(): the library's event slots 9 and 10
    (include/roreg_hip.h), read here and not through hip.PROFILE_SLOTS, which names the learned pipeline's and dense ICP's nine."""
    out = []
    for slot in (9, 10):
        ms, n = ctypes.c_double(0.0), ctypes.c_int(0)
        _check(lib().roreg_profile_read(slot, ctypes.byref(ms), ctypes.byref(n)), 'roreg_profile_read')
        out.append(ms.value)
    return tuple(out)
