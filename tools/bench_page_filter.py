"""Timing of the device page filters (csrc/page_filter.hip: Gaussian blur radius 3, grey edge filter) next to the resize they precede
(csrc/resample.hip, as tools/bench_resample.py times it), on the same pages: a batch of 1024 x 1024 pages and one 4096 x 4096 page, resized to 1024
as generate.py does.  Prints microseconds per page and one JSON line (kept in profiles/page_filter_bench.json).
usage: python tools/bench_page_filter.py [n] [--json PATH]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from layoutdetr_amd.training.dataset_layoutganpp import background_to_tensor, filter_pages

REPS = 10


def graph_us(fn):
    """Microseconds per call: REPS calls captured in one graph (no launch gaps from Python), median of five replays."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            fn()
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); g.replay(); e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) / REPS * 1e3)
    return sorted(times)[len(times) // 2]


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith('--')]
    n = int(argv[0]) if argv else 16
    out_path = sys.argv[sys.argv.index('--json') + 1] if '--json' in sys.argv else None
    dev = torch.device('cuda:0')
    rows = []
    for count, side in ((n, 1024), (1, 4096)):
        pages = torch.randint(0, 256, (count, side, side, 3), dtype=torch.uint8, device=dev)
        row = dict(pages=count, side=side,
                   blur_us_per_page=graph_us(lambda: filter_pages(pages, 'blur', 3.0)) / count,
                   edge_us_per_page=graph_us(lambda: filter_pages(pages, 'edge')) / count,
                   resize_to_1024_us_per_page=graph_us(lambda: background_to_tensor(pages, 1024)) / count,
                   resize_to_256_us_per_page=graph_us(lambda: background_to_tensor(pages, 256)) / count)
        rows.append(row)
        print(f"{count} x {side}x{side}: blur {row['blur_us_per_page']:.1f} us/page, edge {row['edge_us_per_page']:.1f} us/page, "
              f"resize -> 1024 {row['resize_to_1024_us_per_page']:.1f} us/page, resize -> 256 {row['resize_to_256_us_per_page']:.1f} us/page "
              f"(blur = {row['blur_us_per_page'] / row['resize_to_1024_us_per_page']:.2f} x the resize to 1024)")
    line = json.dumps(dict(device=torch.cuda.get_device_name(0), reps_per_graph=REPS, rows=rows))
    print(line)
    if out_path:
        with open(out_path, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
