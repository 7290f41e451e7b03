"""What the tests of the opt-in 16-bit route share (tests/test_h16_cpu.py, tests/test_gpu_conv_h16.py, tests/test_gpu_forward_h16.py):
the two storage types, the single-launch case tables, and the ROUNDING SIMULATION that is the yardstick of whole blocks and networks.

The simulation is a float64 run of an oracle graph (oracle.nets) on the host in which the input, the weights of every Conv2d /
ConvTranspose2d / Linear, and the output of every BatchNorm2d / ReLU / MaxPool2d / PixelShuffle MODULE are rounded to the 16-bit type T
and carried on in float64: every product and sum is (almost) exact, so what it measures against the plain float64 run is the cost of
storing the network's operands and activations in T — the error a correct 16-bit route cannot avoid.  (Functional relu / pixel_shuffle
calls of the oracle graphs need no hook: they map T values to T values.)
"""
import copy

import torch
import torch.nn as nn

U32 = 2.0 ** -24                       # unit round-off of the fp32 accumulation and write-out

# name -> (torch dtype, `dtype` code of the C ABI, half the relative spacing of T, smallest absolute half-spacing that matters)
DTYPES = {
    "fp16": (torch.float16, 0, 2.0 ** -11, 2.0 ** -25),       # subnormal fp16 spacing is 2^-24
    "bf16": (torch.bfloat16, 1, 2.0 ** -8, 0.0),              # bf16 has fp32's range: its subnormals are far below anything here
}


def round_to(t: torch.Tensor, dtype) -> torch.Tensor:
    """Round to the 16-bit type (nearest even, overflow to inf, as tensor.to does) and carry on in the tensor's own float type."""
    return t.to(dtype).to(t.dtype)


# ------------------------------------------------------------------------------------------------------ single-launch cases
def _case(n, cin, cout, h, w, r, stride, pad, bn=True, bias=False, res=False, relu=False, via_converter=False, note=""):
    """`contract`: Cin % 8 == 0 at the C ABI (after the converter's padding when the case goes through it); `t_out`: Cout % 8 == 0, so
    the 16-bit NHWC write-out serves the case (the fp32 NCHW write-out serves every Cout)."""
    cin_abi = (cin + 7) // 8 * 8 if via_converter else cin
    return dict(n=n, cin=cin, cout=cout, h=h, w=w, r=r, stride=stride, pad=pad, bn=bn, bias=bias, res=res, relu=relu, via_converter=via_converter,
                contract=cin_abi % 8 == 0, t_out=cout % 8 == 0, note=note)


CONV_CASES = {
    "stem7x7s2_3to64_9x7": _case(2, 3, 64, 9, 7, 7, 2, 3, relu=True, via_converter=True, note="K = 392 at the ABI: a partial k-tile, padded channels, odd planes"),
    "3x3_16to24_5x3_n3": _case(3, 16, 24, 5, 3, 3, 1, 1, note="M = 45: partial tile in pixels and in channels"),
    "3x3s2_8to24_6x4": _case(2, 8, 24, 6, 4, 3, 2, 1, relu=True, note="even extent under stride 2"),
    "3x3s2_8to24_7x5": _case(2, 8, 24, 7, 5, 3, 2, 1, relu=True, note="odd extent under stride 2"),
    "1x1s2_8to32_5x5": _case(2, 8, 32, 5, 5, 1, 2, 0, note="projection shortcut"),
    "1x1_8to8_1x1_n1": _case(1, 8, 8, 1, 1, 1, 1, 0, note="K = 8, below one MFMA's k"),
    "1x1_32to32_1x1_res_relu": _case(1, 32, 32, 1, 1, 1, 1, 0, res=True, relu=True, note="the SE Linear shape"),
    "3x3_512to16_2x2": _case(2, 512, 16, 2, 2, 3, 1, 1, note="K = 4608, the networks' longest"),
    "3x3_8to8_6x5_n11": _case(11, 8, 8, 6, 5, 3, 1, 1, res=True, relu=True, note="M = 330: 30-pixel images straddle the end of a 64-, 128- and 256-pixel tile"),
    "head1x1_16to17_bias": _case(2, 16, 17, 6, 5, 1, 1, 0, bn=False, bias=True, note="Cout not a multiple of 8: fp32 NCHW only"),
}
NCHW_CASES = ("head1x1_16to17_bias", "stem7x7s2_3to64_9x7", "3x3_16to24_5x3_n3")          # the fp32 NCHW write-out
EXACT_CASES = ("3x3_512to16_2x2", "3x3_8to8_6x5_n11", "stem7x7s2_3to64_9x7")            # integer data, fp32 NCHW write-out
DECONV_CASES = {"deconv_8to8_3x2": (2, 8, 8, 3, 2), "deconv_8to8_1x1": (2, 8, 8, 1, 1)}   # (N, Cin, Cout, H, W): every phase has clipped taps
# what the C ABI refuses: (Cin, Cout, 16-bit output?) — `contract` False by construction
REFUSED_CASES = {"cin12": dict(cin=12, cout=8, t_out=True, contract=False), "cout17_t_out": dict(cin=16, cout=17, t_out=True, contract=False)}
GLUE_PLANES = ((5, 7, 8), (5, 7, 24))                                                     # (H, W, C): odd planes, one and three channel groups


# ------------------------------------------------------------------------------------------------------ rounding simulation
_ROUNDED_WEIGHTS = (nn.Conv2d, nn.ConvTranspose2d, nn.Linear)
_ROUNDED_OUTPUTS = (nn.BatchNorm2d, nn.ReLU, nn.MaxPool2d, nn.PixelShuffle)


def simulation(ref: nn.Module, dtype) -> nn.Module:
    """A float64 eval-mode copy of the oracle graph `ref` with its weights rounded to `dtype` and the rounding hooks in place."""
    sim = copy.deepcopy(ref).double().eval()
    with torch.no_grad():
        for mod in sim.modules():
            if isinstance(mod, _ROUNDED_WEIGHTS):
                mod.weight.copy_(round_to(mod.weight, dtype))
    for mod in sim.modules():
        if isinstance(mod, _ROUNDED_OUTPUTS):
            mod.register_forward_hook(lambda m, inp, out: round_to(out, dtype))
    return sim


def simulate(ref: nn.Module, x, dtype, keep=None):
    """Output of the rounding simulation of `ref` on `x` (a float64 tensor, or a list of them for a multi-branch module), the input rounded
    to `dtype` first.  `keep`: an attribute name of `ref` whose output is returned as well (the trunk, for the embedding)."""
    sim = simulation(ref, dtype)
    kept = {}
    if keep is not None:
        getattr(sim, keep).register_forward_hook(lambda m, inp, out: kept.__setitem__("out", out))
    with torch.no_grad():
        xs = [round_to(t.double(), dtype) for t in x] if isinstance(x, (list, tuple)) else round_to(x.double(), dtype)
        y = sim(xs)
    return (y, kept["out"]) if keep is not None else y
