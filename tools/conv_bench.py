#!/usr/bin/env python3
"""One decoder 3x3 convolution alone (sdvar_op_conv_planes_ex, f16x2 planes, fused GroupNorm statistics as in the decoder): median / min of 20 launches by HIP events.
python tools/conv_bench.py [--lib PATH] [B H W Cin Cout]          default: the level-0 conv, B = 8, 256^2, 160 -> 160
A/B inside one build with SDVAR_CONV_TAP_REUSE=0|1 and SDVAR_CONV_PP (read per call); SDVAR_CONV_DBG needs --lib pointing at a -DSDVAR_TIMING_EXPERIMENTS build."""
import argparse, ctypes as C, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdvar_amd import engine as E
ap = argparse.ArgumentParser(); ap.add_argument("--lib", default=E.LIB_PATH); ap.add_argument("shape", type=int, nargs="*", default=[8, 256, 256, 160, 160])
a = ap.parse_args()
lib = E.load_library(os.path.abspath(a.lib))
B, H, W, Cin, N = a.shape
dev = torch.device("cuda:0")
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
pf = 2
G = (W + 3 + 15) // 16 * 16; R = B * (H + 2) * (W + 2) + 2 * G
x = torch.randn(B * H * W, Cin, device=dev)
xp = torch.zeros((pf, Cin // 32, R, 32), dtype=torch.int16, device=dev)
E._check(lib.sdvar_op_vae_prep(p(x), None, None, None, p(xp), (Cin // 32) * R * 32, pf, B, Cin, H, W, 0, 0, G, st()))
w = (torch.randn(N, Cin, 3, 3, device=dev) / (9 * Cin) ** 0.5).contiguous()
wp = torch.zeros(pf, 9 * Cin // 32, N, 32, dtype=torch.int16, device=dev); wsc = torch.zeros(4, device=dev)
E._check(lib.sdvar_op_conv_weight_planes(p(w), p(wp), N, Cin, 9, 9 * Cin * N, pf, p(wsc), st()))
bias = torch.zeros(N, device=dev)
out = torch.empty(B * H * W, N, device=dev)
part = torch.zeros(B * ((H * W) // 256 + 1) * 64, dtype=torch.float64, device=dev); stats = torch.zeros(B, 32, 2, device=dev)
done = C.c_int32(-1)
def run():
    E._check(lib.sdvar_op_conv_planes_ex(p(xp), (Cin // 32) * R * 32, R, G, p(wp), 9 * Cin * N, pf, p(wsc), p(bias), None, p(out), B, H, W, N, Cin, 9, None, 0, 0, -1, 0,
                                         p(part), p(stats), C.byref(done), st()))
for _ in range(3): run()
torch.cuda.synchronize()
ts = []
for _ in range(20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); run(); e1.record(); e1.synchronize(); ts.append(e0.elapsed_time(e1) * 1e3)
ts.sort()
fl = 2.0 * B * H * W * N * Cin * 9
print(f"conv B={B} {H}x{W} {Cin}->{N} dbg={os.environ.get('SDVAR_CONV_DBG', '0')} reuse={os.environ.get('SDVAR_CONV_TAP_REUSE', '-')}: median {ts[10]:.1f} us, min {ts[0]:.1f} us, "
      f"{fl / ts[10] / 1e6:.1f} TF/s, finite={bool(torch.isfinite(out).all())}")
