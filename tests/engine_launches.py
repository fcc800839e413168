"""Shared by the engine's GPU tests (test_engine_bench_shapes_gpu.py, test_engine_dispatch_gpu.py): record which kernel template the launch
policy of the fp32-operand engine chose for every C-ABI call (ldetr_engine_last_launch through hip.core.engine_call) and compare with a table."""
import os

SWEEP_FORCED = any(k in os.environ.get('LDETR_DEBUG', '') for k in ('FORCE_TILE', 'FORCE_SK', 'SPLIT_BF16', 'GEMM_PAIR', 'SMALL_FAST', 'FAST_LOADS'))


class Launches(object):
    """`with Launches() as L:` records (C-ABI entry, launched kernel template) of every engine call inside (hip.core.engine_call)."""

    def __enter__(self):
        from layoutdetr_amd.hip import core
        self.core = core
        self.was = core.PROF.enabled
        core.PROF.enabled = True
        self.start = len(core.PROF.records)
        return self

    def __exit__(self, *exc):
        self.core.PROF.enabled = self.was
        self.seen = [(r[0].replace('ldetr_', '').replace('_f32', ''), r[6]) for r in self.core.PROF.records[self.start:]]
        del self.core.PROF.records[self.start:]
        return False


def expect(seen, want, what):
    """want: {entry: kernel template}; every listed entry must have launched exactly that template (skipped under the development sweeps'
    forcing switches)."""
    got = {}
    for entry, lab in seen:
        got.setdefault(entry, []).append(lab)
    print(f'  {what}: ' + '; '.join(f'{e} -> {", ".join(l)}' for e, l in got.items()))
    if SWEEP_FORCED or want is None:
        return
    for entry, labs in want.items():
        assert entry in got, f'{what}: no {entry} launch recorded ({got})'
        assert got[entry] == list(labs), f'{what}: {entry} launched {got[entry]}, the bench shape is pinned to {list(labs)}'
