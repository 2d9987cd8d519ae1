"""The binding's refusals of the four pressure nets' training calls, word for word: the ScaleNet and the 16-channel bank net, each in 2D and
3D.  One table of the nets and one body per operation raise them (csrc/fluidnet_cpp.cpp); the texts are those of the per-family bodies the
table replaced, recorded from a build of that code, and differ between the families on purpose (which image sizes the binding knows,
which refusals are the C ABI's).  Nothing is launched by a refused call, so the grids are the nets' smallest: 2D B = 2, 8 x 12; 3D B = 1,
4 x 8 x 12.  A RuntimeError's first line is compared (a build with C++ stack traces appends frames)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# net -> bank, ndim, and the extension's names of pack_t, forward_train, backward, whole_forward_train, whole_backward (stated here and not
# read from the package's table: the texts must not depend on it)
NETS = {"scalenet2d": (False, 2, "scalenet_pack_t multiscale_forward_train multiscale_backward fluidnet_forward_train fluidnet_backward"),
        "scalenet3d": (False, 3, "scalenet3d_pack_t multiscale3d_forward_train multiscale3d_backward fluidnet3d_forward_train fluidnet3d_backward"),
        "bank2d": (True, 2, "banknet_pack_t banknet_forward_train banknet_backward fluidnet_bank_forward_train fluidnet_bank_backward"),
        "bank3d": (True, 3, "banknet3d_pack_t banknet3d_forward_train banknet3d_backward fluidnet_bank3d_forward_train fluidnet_bank3d_backward")}


def _images(ext, bank, ndim, pack_t, dev):
    from fluidnet_cxx_amd.model import _bank_keys, blob_from_state_dict
    from fluidnet_cxx_amd.weights import make_banknet_weights, make_scalenet_weights
    if bank:
        blob = torch.from_numpy(blob_from_state_dict(make_banknet_weights(0, ndim=ndim), keys=_bank_keys())).to(dev)
        return (ext.banknet3d_pack if ndim == 3 else ext.banknet_pack)(blob), pack_t(blob)
    blob = torch.from_numpy(blob_from_state_dict(make_scalenet_weights(0, ndim=ndim), ndim)).to(dev)
    return ext.scalenet_pack(blob, ndim == 3), pack_t(blob)


def refusals(name):
    """{case: first line of the RuntimeError} of every refused call of one net"""
    from fluidnet_cxx_amd._ext import ext
    bank, ndim, names = NETS[name]
    fn = dict(zip(("pack_t", "forward_train", "backward", "whole_forward_train", "whole_backward"), (getattr(ext, n) for n in names.split())))
    dev = torch.device("cuda")
    B, D, H, W = (2, 1, 8, 12) if ndim == 2 else (1, 4, 8, 12)
    g = torch.Generator().manual_seed(5)
    packed, packed_t = _images(ext, bank, ndim, fn["pack_t"], dev)
    inp = torch.randn(B, ndim + 3, D, H, W, generator=g).to(dev)
    inp[:, ndim + 1] = 0.0                                                       # flags: all fluid
    x = torch.randn((B, 2, D, H, W) if ndim == 3 else (B, 2, H, W), generator=g).to(dev)
    # one accepted call of each forward: the tapes, and the scale and flags of the whole forward
    p_net, tape_net = fn["forward_train"](packed, x, "fp32")
    p, U, tape, scale, flags = fn["whole_forward_train"](packed, inp, 1e-5, "fp32")
    gp_net, gp, gU = torch.ones_like(p_net), torch.ones_like(p), torch.ones_like(U)
    xs = (x,) if bank else ()                               # (the bank nets' backward takes the net's input)
    short = torch.zeros(packed.numel() - 256, dtype=torch.uint8, device=dev)
    short_t = torch.zeros(packed_t.numel() - 256, dtype=torch.uint8, device=dev)
    calls = {
        "forward_train: image of the wrong size": lambda: fn["forward_train"](short, x, "fp32"),
        "whole_forward_train: image of the wrong size": lambda: fn["whole_forward_train"](short, inp, 1e-5, "fp32"),
        "backward: image of the wrong size": lambda: fn["backward"](short_t, *xs, gp_net, tape_net, "fp32"),
        "whole_backward: image of the wrong size": lambda: fn["whole_backward"](short_t, flags, scale, gp, gU, tape, "fp32"),
        "forward_train: packed_t for packed": lambda: fn["forward_train"](packed_t, x, "fp32"),
        "whole_forward_train: packed_t for packed": lambda: fn["whole_forward_train"](packed_t, inp, 1e-5, "fp32"),
        "backward: packed for packed_t": lambda: fn["backward"](packed, *xs, gp_net, tape_net, "fp32"),
        "whole_backward: packed for packed_t": lambda: fn["whole_backward"](packed, flags, scale, gp, gU, tape, "fp32"),
        "backward: tape of the wrong length": lambda: fn["backward"](packed_t, *xs, gp_net, tape_net[:-1], "fp32"),
        "whole_backward: tape of the wrong length": lambda: fn["whole_backward"](packed_t, flags, scale, gp, gU, tape[:-1], "fp32"),
        "whole_backward: grad_U on another grid": lambda: fn["whole_backward"](packed_t, flags, scale, gp, gU[..., :-4].contiguous(), tape, "fp32"),
        "whole_backward: flags on another grid": lambda: fn["whole_backward"](packed_t, flags[..., :-4, :].contiguous(), scale, gp, gU, tape, "fp32"),
        "whole_backward: grad_p on another grid": lambda: fn["whole_backward"](packed_t, flags, scale, torch.ones_like(gp[..., :-4]), gU, tape, "fp32"),
        "whole_backward: scale of the wrong length": lambda: fn["whole_backward"](packed_t, flags, torch.ones(B + 1, device=dev), gp, gU, tape, "fp32"),
        "forward_train: unknown precision_mode": lambda: fn["forward_train"](packed, x, "fp64"),
        "whole_forward_train: unknown precision_mode": lambda: fn["whole_forward_train"](packed, inp, 1e-5, "fp64"),
        "backward: unknown precision_mode": lambda: fn["backward"](packed_t, *xs, gp_net, tape_net, "fp64"),
        "whole_backward: unknown precision_mode": lambda: fn["whole_backward"](packed_t, flags, scale, gp, gU, tape, "fp64"),
        "forward_train: bf16x6": lambda: fn["forward_train"](packed, x, "bf16x6"),
        "whole_forward_train: bf16x3": lambda: fn["whole_forward_train"](packed, inp, 1e-5, "bf16x3"),
        "backward: bf16x3": lambda: fn["backward"](packed_t, *xs, gp_net, tape_net, "bf16x3"),
        "whole_backward: bf16x6": lambda: fn["whole_backward"](packed_t, flags, scale, gp, gU, tape, "bf16x6"),
    }
    if bank:
        calls["backward: x on another grid"] = lambda: fn["backward"](packed_t, x[..., :-4].contiguous(), gp_net, tape_net, "fp32")
    else:
        plain = getattr(ext, names.split()[2] + "_plain")
        calls["backward_plain: packed for packed_t"] = lambda: plain(packed, gp_net, tape_net, "fp32")
        calls["backward_plain: tape of the wrong length"] = lambda: plain(packed_t, gp_net, tape_net[:-1], "fp32")
    out = {}
    for case, call in calls.items():
        try:
            call()
            out[case] = "(not refused)"
        except RuntimeError as e:
            out[case] = str(e).split("\n")[0]
    torch.cuda.synchronize()
    return out


# the texts, recorded from a build of the per-family bodies (one process, these grids)
EXPECTED = {
    "bank2d": {
        "backward: bf16x3": "fnx_banknet_backward: the bank net runs in fp32 arithmetic only (FNX_PRECISION_FP32, _FP32_F4,"
            " _FP32_F2 or _FP32_DIRECT), not in the bf16 modes (precision_mode 3)",
        "backward: image of the wrong size": "packed_t must be the 20608-byte image from banknet_pack_t on the input's device (got 20352 bytes)",
        "backward: packed for packed_t": "packed_t must be the 20608-byte image from banknet_pack_t on the input's device (got 23040 bytes)",
        "backward: tape of the wrong length": "tape has 23231 floats, not the layout of this grid",
        "backward: unknown precision_mode": "precision_mode must be 'fp32', 'fp32_direct', 'fp32_f4', 'fp32_f2', 'bf16x6' or 'bf16x3', got 'fp64'",
        "backward: x on another grid": "grad_p (1 channel) and x (2 channels) must share their grid",
        "forward_train: bf16x6": "fnx_banknet_forward_train: the bank net runs in fp32 arithmetic only (FNX_PRECISION_FP32, _FP32_F4,"
            " _FP32_F2 or _FP32_DIRECT), not in the bf16 modes (precision_mode 2)",
        "forward_train: image of the wrong size": "packed must be the 23040-byte image from banknet_pack (got 22784 bytes)",
        "forward_train: packed_t for packed": "packed must be the 23040-byte image from banknet_pack (got 20608 bytes)",
        "forward_train: unknown precision_mode": "precision_mode must be 'fp32', 'fp32_direct', 'fp32_f4', 'fp32_f2', 'bf16x6' or 'bf16x3', got"
            " 'fp64'",
        "whole_backward: bf16x6": "fnx_fluidnet_bank_backward: the bank net runs in fp32 arithmetic only (FNX_PRECISION_FP32,"
            " _FP32_F4, _FP32_F2 or _FP32_DIRECT), not in the bf16 modes (precision_mode 2)",
        "whole_backward: flags on another grid": "grad_p, grad_U and flags must share their grid",
        "whole_backward: grad_U on another grid": "grad_p, grad_U and flags must share their grid",
        "whole_backward: grad_p on another grid": "grad_p, grad_U and flags must share their grid",
        "whole_backward: image of the wrong size": "packed_t must be the 20608-byte image from banknet_pack_t on the input's device (got 20352"
            " bytes)",
        "whole_backward: packed for packed_t": "packed_t must be the 20608-byte image from banknet_pack_t on the input's device (got 23040 bytes)",
        "whole_backward: scale of the wrong length": "scale must hold B floats on the GPU",
        "whole_backward: tape of the wrong length": "tape has 23231 floats, not the layout of this grid",
        "whole_backward: unknown precision_mode": "precision_mode must be 'fp32', 'fp32_direct', 'fp32_f4', 'fp32_f2', 'bf16x6' or 'bf16x3', got"
            " 'fp64'",
        "whole_forward_train: bf16x3": "fnx_fluidnet_bank_forward_train: the bank net runs in fp32 arithmetic only (FNX_PRECISION_FP32,"
            " _FP32_F4, _FP32_F2 or _FP32_DIRECT), not in the bf16 modes (precision_mode 3)",
        "whole_forward_train: image of the wrong size": "packed must be the 23040-byte image from banknet_pack (got 22784 bytes)",
        "whole_forward_train: packed_t for packed": "packed must be the 23040-byte image from banknet_pack (got 20608 bytes)",
        "whole_forward_train: unknown precision_mode": "precision_mode must be 'fp32', 'fp32_direct', 'fp32_f4', 'fp32_f2', 'bf16x6' or 'bf16x3', got"
            " 'fp64'",
    },
    "bank3d": {
        "backward: bf16x3": "fnx_banknet3d_backward: the bank net runs in fp32 arithmetic only (FNX_PRECISION_FP32, _FP32_F4,"
            " _FP32_F2 or _FP32_DIRECT), not in the bf16 modes (precision_mode 3)",
        "backward: image of the wrong size": "packed_t must be the 57472-byte image from banknet3d_pack_t on the input's device (got 57216 bytes)",
        "backward: packed for packed_t": "packed_t must be the 57472-byte image from banknet3d_pack_t on the input's device (got 62208 bytes)",
        "backward: tape of the wrong length": "tape has 43391 floats, not the layout of this grid",
        "backward: unknown precision_mode": "precision_mode must be 'fp32', 'fp32_direct', 'fp32_f4', 'fp32_f2', 'bf16x6' or 'bf16x3', got 'fp64'",
        "backward: x on another grid": "grad_p (1 channel) and x (2 channels) must share their grid",
        "forward_train: bf16x6": "fnx_banknet3d_forward_train: the bank net runs in fp32 arithmetic only (FNX_PRECISION_FP32,"
            " _FP32_F4, _FP32_F2 or _FP32_DIRECT), not in the bf16 modes (precision_mode 2)",
        "forward_train: image of the wrong size": "packed must be the 62208-byte image from banknet3d_pack (got 61952 bytes)",
        "forward_train: packed_t for packed": "packed must be the 62208-byte image from banknet3d_pack (got 57472 bytes)",
        "forward_train: unknown precision_mode": "precision_mode must be 'fp32', 'fp32_direct', 'fp32_f4', 'fp32_f2', 'bf16x6' or 'bf16x3', got"
            " 'fp64'",
        "whole_backward: bf16x6": "fnx_fluidnet_bank3d_backward: the bank net runs in fp32 arithmetic only (FNX_PRECISION_FP32,"
            " _FP32_F4, _FP32_F2 or _FP32_DIRECT), not in the bf16 modes (precision_mode 2)",
        "whole_backward: flags on another grid": "grad_p, grad_U and flags must share their grid",
        "whole_backward: grad_U on another grid": "grad_p, grad_U and flags must share their grid",
        "whole_backward: grad_p on another grid": "grad_p, grad_U and flags must share their grid",
        "whole_backward: image of the wrong size": "packed_t must be the 57472-byte image from banknet3d_pack_t on the input's device (got 57216"
            " bytes)",
        "whole_backward: packed for packed_t": "packed_t must be the 57472-byte image from banknet3d_pack_t on the input's device (got 62208 bytes)",
        "whole_backward: scale of the wrong length": "scale must hold B floats on the GPU",
        "whole_backward: tape of the wrong length": "tape has 43391 floats, not the layout of this grid",
        "whole_backward: unknown precision_mode": "precision_mode must be 'fp32', 'fp32_direct', 'fp32_f4', 'fp32_f2', 'bf16x6' or 'bf16x3', got"
            " 'fp64'",
        "whole_forward_train: bf16x3": "fnx_fluidnet_bank3d_forward_train: the bank net runs in fp32 arithmetic only (FNX_PRECISION_FP32,"
            " _FP32_F4, _FP32_F2 or _FP32_DIRECT), not in the bf16 modes (precision_mode 3)",
        "whole_forward_train: image of the wrong size": "packed must be the 62208-byte image from banknet3d_pack (got 61952 bytes)",
        "whole_forward_train: packed_t for packed": "packed must be the 62208-byte image from banknet3d_pack (got 57472 bytes)",
        "whole_forward_train: unknown precision_mode": "precision_mode must be 'fp32', 'fp32_direct', 'fp32_f4', 'fp32_f2', 'bf16x6' or 'bf16x3', got"
            " 'fp64'",
    },
    "scalenet2d": {
        "backward: bf16x3": "fnx_multiscale_backward: training runs in fp32 arithmetic only (FNX_PRECISION_FP32, _FP32_F4,"
            " _FP32_F2 or _FP32_DIRECT), not in the bf16 modes (precision_mode 3)",
        "backward: image of the wrong size": "packed_t must be the 14793984-byte image from scalenet_pack_t (got 14793728 bytes)",
        "backward: packed for packed_t": "packed_t must be the 14793984-byte image from scalenet_pack_t (got 12622080 bytes)",
        "backward: tape of the wrong length": "tape has 81855 floats, not the layout of this grid",
        "backward: unknown precision_mode": "precision_mode must be 'fp32', 'fp32_direct', 'fp32_f4', 'fp32_f2', 'bf16x6' or 'bf16x3', got 'fp64'",
        "backward_plain: packed for packed_t": "packed_t must be the 14793984-byte image from scalenet_pack_t (got 12622080 bytes)",
        "backward_plain: tape of the wrong length": "tape has 81855 floats, not the layout of this grid",
        "forward_train: bf16x6": "fnx_multiscale_forward_train: training runs in fp32 arithmetic only (FNX_PRECISION_FP32, _FP32_F4,"
            " _FP32_F2 or _FP32_DIRECT), not in the bf16 modes (precision_mode 2)",
        "forward_train: image of the wrong size": "packed must be the 12622080-byte image from scalenet_pack (got 12621824 bytes)",
        "forward_train: packed_t for packed": "packed must be the 12622080-byte image from scalenet_pack (got 14793984 bytes)",
        "forward_train: unknown precision_mode": "precision_mode must be 'fp32', 'fp32_direct', 'fp32_f4', 'fp32_f2', 'bf16x6' or 'bf16x3', got"
            " 'fp64'",
        "whole_backward: bf16x6": "fnx_fluidnet_backward: training runs in fp32 arithmetic only (FNX_PRECISION_FP32, _FP32_F4,"
            " _FP32_F2 or _FP32_DIRECT), not in the bf16 modes (precision_mode 2)",
        "whole_backward: flags on another grid": "grad_p, grad_U and flags must share their grid",
        "whole_backward: grad_U on another grid": "grad_p, grad_U and flags must share their grid",
        "whole_backward: grad_p on another grid": "grad_p, grad_U and flags must share their grid",
        "whole_backward: image of the wrong size": "packed_t must be the 14793984-byte image from scalenet_pack_t (got 14793728 bytes)",
        "whole_backward: packed for packed_t": "packed_t must be the 14793984-byte image from scalenet_pack_t (got 12622080 bytes)",
        "whole_backward: scale of the wrong length": "scale must hold B floats on the GPU",
        "whole_backward: tape of the wrong length": "tape has 81855 floats, not the layout of this grid",
        "whole_backward: unknown precision_mode": "precision_mode must be 'fp32', 'fp32_direct', 'fp32_f4', 'fp32_f2', 'bf16x6' or 'bf16x3', got"
            " 'fp64'",
        "whole_forward_train: bf16x3": "fnx_fluidnet_forward_train: training runs in fp32 arithmetic only (FNX_PRECISION_FP32, _FP32_F4,"
            " _FP32_F2 or _FP32_DIRECT), not in the bf16 modes (precision_mode 3)",
        "whole_forward_train: image of the wrong size": "packed must be the 12622080-byte image from scalenet_pack (got 12621824 bytes)",
        "whole_forward_train: packed_t for packed": "packed must be the 12622080-byte image from scalenet_pack (got 14793984 bytes)",
        "whole_forward_train: unknown precision_mode": "precision_mode must be 'fp32', 'fp32_direct', 'fp32_f4', 'fp32_f2', 'bf16x6' or 'bf16x3', got"
            " 'fp64'",
    },
    "scalenet3d": {
        "backward: bf16x3": "fnx_multiscale3d_backward: training runs in fp32 arithmetic only (FNX_PRECISION_FP32, _FP32_F4,"
            " _FP32_F2 or _FP32_DIRECT), not in the bf16 modes (precision_mode 3)",
        "backward: image of the wrong size": "fnx_multiscale3d_backward: the weight image has 43572224 bytes, not the 43572480 of"
            " fnx_scalenet3d_pack_t",
        "backward: packed for packed_t": "fnx_multiscale3d_backward: the weight image has 38030592 bytes, not the 43572480 of"
            " fnx_scalenet3d_pack_t (packed and packed3d_t are swapped)",
        "backward: tape of the wrong length": "tape has 144639 floats, not the layout of this grid",
        "backward: unknown precision_mode": "precision_mode must be 'fp32', 'fp32_direct', 'fp32_f4', 'fp32_f2', 'bf16x6' or 'bf16x3', got 'fp64'",
        "backward_plain: packed for packed_t": "fnx_multiscale3d_backward_plain: the weight image has 38030592 bytes, not the 43572480 of"
            " fnx_scalenet3d_pack_t (packed and packed3d_t are swapped)",
        "backward_plain: tape of the wrong length": "tape has 144639 floats, not the layout of this grid",
        "forward_train: bf16x6": "fnx_multiscale3d_forward_train: training runs in fp32 arithmetic only (FNX_PRECISION_FP32,"
            " _FP32_F4, _FP32_F2 or _FP32_DIRECT), not in the bf16 modes (precision_mode 2)",
        "forward_train: image of the wrong size": "fnx_multiscale3d_forward_train: the weight image has 38030336 bytes, not the 38030592 of"
            " fnx_scalenet_pack(is3D = 1)",
        "forward_train: packed_t for packed": "fnx_multiscale3d_forward_train: the weight image has 43572480 bytes, not the 38030592 of"
            " fnx_scalenet_pack(is3D = 1) (packed and packed3d_t are swapped)",
        "forward_train: unknown precision_mode": "precision_mode must be 'fp32', 'fp32_direct', 'fp32_f4', 'fp32_f2', 'bf16x6' or 'bf16x3', got"
            " 'fp64'",
        "whole_backward: bf16x6": "fnx_fluidnet3d_backward: training runs in fp32 arithmetic only (FNX_PRECISION_FP32, _FP32_F4,"
            " _FP32_F2 or _FP32_DIRECT), not in the bf16 modes (precision_mode 2)",
        "whole_backward: flags on another grid": "grad_p, grad_U and flags must share their grid",
        "whole_backward: grad_U on another grid": "grad_p, grad_U and flags must share their grid",
        "whole_backward: grad_p on another grid": "grad_p, grad_U and flags must share their grid",
        "whole_backward: image of the wrong size": "fnx_fluidnet3d_backward: the weight image has 43572224 bytes, not the 43572480 of"
            " fnx_scalenet3d_pack_t",
        "whole_backward: packed for packed_t": "fnx_fluidnet3d_backward: the weight image has 38030592 bytes, not the 43572480 of"
            " fnx_scalenet3d_pack_t (packed and packed3d_t are swapped)",
        "whole_backward: scale of the wrong length": "scale must hold B floats on the GPU",
        "whole_backward: tape of the wrong length": "tape has 144639 floats, not the layout of this grid",
        "whole_backward: unknown precision_mode": "precision_mode must be 'fp32', 'fp32_direct', 'fp32_f4', 'fp32_f2', 'bf16x6' or 'bf16x3', got"
            " 'fp64'",
        "whole_forward_train: bf16x3": "fnx_fluidnet3d_forward_train: training runs in fp32 arithmetic only (FNX_PRECISION_FP32, _FP32_F4,"
            " _FP32_F2 or _FP32_DIRECT), not in the bf16 modes (precision_mode 3)",
        "whole_forward_train: image of the wrong size": "fnx_fluidnet3d_forward_train: the weight image has 38030336 bytes, not the 38030592 of"
            " fnx_scalenet_pack(is3D = 1)",
        "whole_forward_train: packed_t for packed": "fnx_fluidnet3d_forward_train: the weight image has 43572480 bytes, not the 38030592 of"
            " fnx_scalenet_pack(is3D = 1) (packed and packed3d_t are swapped)",
        "whole_forward_train: unknown precision_mode": "precision_mode must be 'fp32', 'fp32_direct', 'fp32_f4', 'fp32_f2', 'bf16x6' or 'bf16x3', got"
            " 'fp64'",
    },
}


@pytest.mark.parametrize("name", sorted(NETS))
def test_refusal_texts(name):
    got = refusals(name)
    for case in sorted(got):
        print(f"{name} | {case} | {got[case]}")
    assert got == EXPECTED[name]
