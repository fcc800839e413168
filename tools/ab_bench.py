#!/usr/bin/env python
"""Step time of two builds of the kernel library, alternating in one call on one GPU (the Python side is the same, only LDETR_LIB differs):

    python tools/ab_bench.py --parent layoutdetr_amd/lib/variants/libldetr_hip_parent.so --runs 7 --out ab.json [-- bench.py arguments]

or, when the Python side changed as well, of two trees (`--parent-tree DIR`: a built checkout of the parent commit; its own bench.py runs there):

    python tools/ab_bench.py --parent-tree ../parent --runs 7 --out ab.json [-- bench.py arguments]

runs `python bench.py --gpus 1 --steps 20 --warmup 5 <arguments>` `--runs` times per build, parent first, each run in a fresh process under its own
time limit; stops at the first run that fails.  Writes every run's ms_per_step, the medians, the ranges and whether the ranges overlap.  The parent
library is the parent commit's `python -m layoutdetr_amd.build` output, copied next to the tree's (tools/build_variant.sh's folder)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one_run(lib, extra, limit, tree=None):
    env = dict(os.environ)
    if lib:
        env['LDETR_LIB'] = os.path.abspath(lib)
    else:
        env.pop('LDETR_LIB', None)
    root = os.path.abspath(tree) if tree else ROOT
    cmd = [sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5'] + extra
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f'bench.py failed with status {r.returncode} ({lib or "this tree"}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
    line = [l for l in r.stdout.splitlines() if l.startswith('{') and '"ms_per_step"' in l][-1]
    return json.loads(line)['ms_per_step']


def summary(runs):
    return dict(runs=runs, median=round(statistics.median(runs), 3), min=min(runs), max=max(runs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', help="the parent commit's libldetr_hip.so")
    ap.add_argument('--parent-tree', help="a built checkout of the parent commit (instead of --parent, when the Python side differs too)")
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--limit', type=int, default=150, help='seconds per run')
    ap.add_argument('--out', required=True)
    ap.add_argument('extra', nargs='*', help='arguments passed on to bench.py (after --)')
    args = ap.parse_args()
    if bool(args.parent) == bool(args.parent_tree):
        ap.error('give one of --parent and --parent-tree')
    parent, this = [], []
    for k in range(args.runs):
        parent.append(one_run(args.parent, args.extra, args.limit, tree=args.parent_tree))
        this.append(one_run(None, args.extra, args.limit))
        print(f'run {k}: parent {parent[-1]:.3f} ms, this tree {this[-1]:.3f} ms', flush=True)
        out = dict(command='python bench.py --gpus 1 --steps 20 --warmup 5 ' + ' '.join(args.extra), unit='ms per step', parent=summary(parent), this=summary(this))
        out['ranges_overlap'] = not (out['this']['max'] < out['parent']['min'] or out['parent']['max'] < out['this']['min'])
        out['median_gain_ms'] = round(out['parent']['median'] - out['this']['median'], 3)
        with open(args.out, 'w') as f:      # rewritten after every pair: a run that is cut short keeps what it measured
            json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ('ranges_overlap', 'median_gain_ms')}))


if __name__ == '__main__':
    main()
