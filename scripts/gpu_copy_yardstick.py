"""The yardstick of the counting pass that writes the text (text_build.hip k_row_count / k_row_count_fast): a device-to-device
copy of m * n bytes, timed with HIP events.  usage: python3 scripts/gpu_copy_yardstick.py [ROWS COLS [REPEATS]]"""
import sys

import torch

m, n = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (1000, 1_000_000)
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
dev = torch.device("cuda:0")
src = torch.randint(0, 255, (m * n,), dtype=torch.uint8, device=dev)
dst = torch.empty(m * n + m + 65, dtype=torch.uint8, device=dev)      # the text's size: a row and its '#', the sentinel, the padding
for _ in range(3):
    dst[:m * n].copy_(src)
torch.cuda.synchronize()
times = []
for _ in range(reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    dst[:m * n].copy_(src)
    b.record()
    b.synchronize()
    times.append(a.elapsed_time(b) * 1e3)
times.sort()
us = times[len(times) // 2]
print(f"d2d copy of {m} x {n} bytes: median {us:.0f} us, min {times[0]:.0f}, max {times[-1]:.0f} over {reps} copies; "
      f"{2 * m * n / us / 1e6:.2f} TB/s read + written")
