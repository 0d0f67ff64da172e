import torch, sys, os
sys.path.insert(0, os.getcwd())
from svnet_amd import _lib, _ops
from svnet_amd._ops import _p, _stream, call
x = torch.randn(32768, 3, 170, device="cuda")
sums = torch.zeros(_ops._sliced_len(340), dtype=torch.float64, device="cuda")
for it in range(3):
    sums.zero_()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(10):
        call("svnet_colstats_f64", _p(x), 32768, 170, 1, _p(sums), _stream())
    b.record()
    torch.cuda.synchronize()
print("us per call", a.elapsed_time(b) * 100)
