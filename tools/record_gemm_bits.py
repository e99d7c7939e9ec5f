"""Record what the irrep GEMM family (csrc/fourier.hip) returns, bit for bit, so that a restructuring of its kernels can be shown to change nothing.

    python tools/record_gemm_bits.py [--out tests/golden/gemm_parent_bits.npz]

Runs a fixed case set on the GPU and writes one sha1 digest per returned tensor (the output coefficients, and the propagated bound where
the case asks for it) and the hash of the commit whose kernels produced them.  Neither inputs nor outputs are stored: the operands come
from seeded numpy generators (weights are drawn directly as the five padded float32 matrices, so no host transform stands between the seed
and the packed operand).  Runs in a git checkout only, and refuses while roreg_amd/csrc or include differ from HEAD: the library must be
that commit's.  tests/test_hip_fourier.py::test_refactor_keeps_the_parents_gemm_bits recomputes run_cases() and compares every digest.

The case set (the smallest shapes at which the kernels' shared pieces can go wrong); layers are (C, O):
  (32, 256)    K = 32, 96, 96, 128, 160 over the five irreps: a single K32 step (the prologue's clamped look-ahead), odd and even step counts
  (64, 256)    two steps, exactly what the prologue requests
  (256, 512)   the BIG instantiations
  (512, 256)   a long loop under a residual
  (64, 64)     128-row tiles, the four-wave generic kernel
  (256, 32), (32, 32), and (32, 256) in word layout: the thin kernels
batches: 32 (one column tile, mostly empty; the half-tile form's right half is empty), 256 (exact), 288 (a ragged last tile whose right
half is empty for d = 1), and 1312 for (32, 256) / 608 for (256, 512): more tiles than the persistent form launches workgroups.
forms, each with and without the residual and with and without the propagated bound where the form takes them: the word layout for every
layer (the thin kernels switched on and off for the thin shapes); the half-block layout on the 32x32x16 and the 16x16x32 kernel for
O % 256 == 0, the latter launched per tile, persistent and on half tiles; bf16 x 3 and plain f32 for (64, 64).
(The ROREG_GEMM_PIPE=0 loop needs a process of its own: tests/test_hip_kernels.py pins it to the pipelined loop.)"""
import argparse
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'gemm_parent_bits.npz')
LAYERS = [(32, 256), (64, 256), (256, 512), (512, 256), (64, 64), (256, 32), (32, 32)]
BATCHES = [32, 256, 288]
WALK_BATCH = {(32, 256): 1312, (256, 512): 608}          # persistent workgroups walk more than one tile (checked against the tile list below)
FLOAT_LAYER = (64, 64)                                   # the bf16 x 3 and the plain f32 kernel
DIMS = (1, 3, 3, 4, 5)


def _digest(t):
    return hashlib.sha1(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def _weights(C, O):
    """the five padded float32 matrices [round_up(d O, 128), d C] of a layer, straight from the generator"""
    rng = np.random.default_rng(1000 * C + O)
    out = []
    for d in DIMS:
        Wp = np.zeros(((d * O + 127) // 128 * 128, d * C), np.float32)
        Wp[:d * O] = (rng.standard_normal((d * O, d * C)) / np.sqrt(d * C)).astype(np.float32)
        out.append(Wp)
    return out


def run_cases():
    """-> {name: sha1 hex digest}: '<case>' for the coefficients, '<case>/bound' for the propagated bound, from the library roreg_amd.hip loads."""
    import torch

    from roreg_amd import hip
    out = {}
    for C, O in LAYERS:
        dense = _weights(C, O)
        w_exp = hip.f16_scale_exp(max(float(np.abs(Wp).max()) for Wp in dense))
        w2 = ([hip.f16_split2_pack(Wp, w_exp) for Wp in dense], w_exp)
        planes_ok = O % 256 == 0
        thin = O == 32 or C == 32
        for B in BATCHES + ([WALK_BATCH[(C, O)]] if (C, O) in WALK_BATCH else []):
            rng = np.random.default_rng(7 * C + 3 * O + B)
            n = hip.coef_size(C, B)
            X = torch.from_numpy((rng.standard_normal(n) * np.exp(rng.standard_normal(n))).astype(np.float32)).cuda()
            add = torch.from_numpy(rng.standard_normal(hip.coef_size(O, B)).astype(np.float32)).cuda()
            nb = (torch.from_numpy(rng.uniform(0.5, 1.5, O).astype(np.float32)).cuda(), torch.from_numpy(rng.uniform(0.0, 1.0, O).astype(np.float32)).cuda())
            Xw, xb = hip.pack_coefs_f16x2(X, C, B)
            Xp = hip.words_to_planes(Xw, C, B) if planes_ok else None
            if B in WALK_BATCH.values():
                assert hip.lib().roreg_irrep_gemm_tiles_m(O, hip.coef_pitch(B), 256, None) > 256, (C, O, B)

            def f16x2(name, Xin, x_planes):
                for a in (None, add):
                    for bound in (None, nb):
                        r = hip.irrep_gemm(Xin, None, C, O, B, f16x2=w2, x_bound=xb, add=a, next_bound=bound, x_planes=x_planes)
                        key = f'{C}x{O}/B{B}/{name}/add{int(a is not None)}/bound{int(bound is not None)}'
                        if bound is None:
                            out[key] = _digest(r)
                        else:
                            out[key], out[key + '/bound'] = _digest(r[0]), _digest(r[1])

            for on in ((1, 0) if thin else (1,)):
                with hip.gemm_thin(on):
                    f16x2(f'words/thin{on}' if thin else 'words', Xw, 0)
            if planes_ok:
                f16x2('planes1', Xp, 1)
                for form in (0, 1, 2):
                    with hip.gemm_persistent(form):
                        f16x2(f'planes2/persist{form}', Xp, 2)
            if (C, O) == FLOAT_LAYER:
                wsplit = [hip.bf16_split3_pack(Wp) for Wp in dense]
                wpack = [hip.pack_conv_weights(torch.from_numpy(Wp).reshape(Wp.shape[0], Wp.shape[1], 1)) for Wp in dense]
                for a in (None, add):
                    out[f'{C}x{O}/B{B}/bf16x3/add{int(a is not None)}'] = _digest(hip.irrep_gemm(X, wpack, C, O, B, split=wsplit, add=a))
                    out[f'{C}x{O}/B{B}/f32/add{int(a is not None)}'] = _digest(hip.irrep_gemm(X, wpack, C, O, B, add=a))
    return out


def save(path, commit, digests):
    """the fixture: the case names, their digests as raw bytes [n][20], the commit"""
    names = sorted(digests)
    np.savez_compressed(path, commit=np.array(commit), names=np.array(names), sha1=np.array([list(bytes.fromhex(digests[k])) for k in names], np.uint8))


def load(path=FIXTURE):
    """-> (commit, {name: sha1 hex digest}) of a recorded fixture"""
    z = np.load(path)
    return str(z['commit']), {str(k): bytes(v).hex() for k, v in zip(z['names'], z['sha1'])}


def clean_commit(tool):
    """the hash of HEAD; exits unless this is a git checkout whose kernels are that commit's (shared with tools/record_conv_bits.py)"""
    git = lambda *args: subprocess.run(('git', '-C', ROOT) + args, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    commit = git('rev-parse', 'HEAD').stdout.strip()
    if len(commit) != 40 or git('diff', '--quiet', 'HEAD', '--', 'roreg_amd/csrc', 'include').returncode != 0:
        sys.exit(f'{tool}: not a git checkout, or roreg_amd/csrc or include differ from HEAD -- the fixture is recorded from committed kernels only')
    return commit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=FIXTURE)
    a = ap.parse_args()
    commit = clean_commit('record_gemm_bits')
    digests = run_cases()
    save(a.out, commit, digests)
    print(f'{a.out}: {len(digests)} digests, {os.path.getsize(a.out)} bytes; commit {commit}')


if __name__ == '__main__':
    main()
