#!/usr/bin/env python3
"""Writes tests/golden/gemm_workspace_bytes.json: emo_gemm_workspace_bytes() of the library it is pointed at, on the grid of shapes that
tests/test_gemm_route_host.py compares against.  The function needs no GPU.  The committed file was written from a build of the commit BEFORE the
GEMM planner (emo_gemm_plan.h) existed, so that the planner's sizes are held to the sizes of the hand-written arithmetic it replaced:

    make -C emo-disentanger_amd/csrc && python tools/gemm_workspace_golden.py emo-disentanger_amd/libemo_hip.so

Entries: [M, N, K, dtype_in, dtype_out, switches, bytes]; dtypes 0 = fp32, 1 = bf16; switches: index into "envs"."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = [{}, {'EMO_W128_TN_MINKT': '1', 'EMO_W128_TN_MINBLK': '1'}, {'EMO_GEMM_W128': '1'}]


def shapes():
    """(M, N, K, switches): the route-table shapes of tests/test_gpu_gemm_exact.py, then every (M, N, K) a training step can ask for."""
    s = []
    s += [(200, 136, K, 0) for K in (128, 160, 512, 576)] + [(129, 8328, K, 0) for K in (32, 64, 96, 128, 1088)] + [(8328, 1024, 64, 0), (300, 264, 128, 0)]
    s += [(M, N, K, 0) for M, N in ((8, 8), (8, 327), (129, 8), (129, 327)) for K in (64, 160)]
    s += [(70, 50, 37, 0), (200, 136, 264, 0), (5, 50, 64, 0), (70, 6, 64, 0), (3, 4, 64, 0)]
    s += [(M, N, K, 0) for M in (1, 17, 32) for N in (8, 24, 327) for K in (32, 96, 160, 512, 1024, 1056, 2048, 2080)]
    s += [(M, N, 512, 0) for M in (4096, 4224) for N in (64, 128, 512, 2048)]
    s += [(M, N, K, e) for M, N, K in ((256, 256, 256), (512, 256, 320), (256, 512, 1088)) for e in (0, 2)]
    s += [(1024, 768, 8192, 0)]
    s += [(M, N, K, e) for M, N, K in ((256, 256, 4096), (256, 512, 4096), (768, 256, 4096), (256, 1280, 4096), (512, 768, 4096), (768, 1024, 2048), (768, 1024, 8192))
          for e in (0, 1)]
    s += [(136, 264, 1024, 0), (136, 264, 8192, 0), (128, 128, 1024, 0), (2048, 512, 2048, 0)]
    s += [(128, 128, 16, 0), (129, 327, 509, 0), (136, 72, 4224, 0), (136, 264, 4224, 0)]
    # training steps: Performer at batch sizes 4 and 64 (T = 2048), GPT-2 at 16, stage 1 at 4 x 512 tokens; model widths, vocabularies (padded and not)
    dims = (200, 256, 327, 384, 512, 1536, 2048)
    for R in (8192, 131072, 32768, 2048):
        s += [(R, a, b, 0) for a in dims for b in dims] + [(a, b, R, 0) for a in dims for b in dims]
    s += [(512, 6144, 512, 0), (6144, 512, 512, 0)]
    return sorted(set(s))


def main(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    f = lib.emo_gemm_workspace_bytes
    f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_int64] * 3 + [ctypes.c_int] * 2
    rows = []
    for M, N, K, e in shapes():
        for k in ENVS[e]:
            os.environ[k] = ENVS[e][k]
        for di, do in ((1, 1), (1, 0), (0, 0)):
            rows.append([M, N, K, di, do, e, f(M, N, K, di, do)])
        for k in ENVS[e]:
            del os.environ[k]
    out = os.path.join(ROOT, 'tests', 'golden', 'gemm_workspace_bytes.json')
    with open(out, 'w') as fh:
        fh.write('{"comment": "emo_gemm_workspace_bytes of the commit before csrc/emo_gemm_plan.h; written by tools/gemm_workspace_golden.py (see its docstring)",\n')
        fh.write(' "envs": %s,\n "rows": [\n' % json.dumps(ENVS))
        fh.write(',\n'.join('  ' + json.dumps(r) for r in rows))
        fh.write('\n ]}\n')
    print('%d rows -> %s' % (len(rows), out))


if __name__ == '__main__':
    main(sys.argv[1])
