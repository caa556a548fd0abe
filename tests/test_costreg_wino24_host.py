"""The F(2x4, 3x3) form of a stride-1 CostRegNet2D layer (csrc/costreg2d_wino24.hip), host side, no GPU: the transform matrices, the
order of packing.pack_reg_layer_wino24's fragments, the accumulator position that carries the bias, and where the new blocks sit
in the network's weight blob."""
import pytest
import torch

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, packing, synth

F64 = torch.float64
BT2 = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=F64)
AT2 = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=F64)
BT4 = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                    [0, 4, 0, -5, 0, 1]], dtype=F64)
AT4 = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=F64)


def unpack(pk, D):
    """The packed array -> U [i 4][j 6][cout][cin] in float64: two arrays of A fragments, patch columns 0-3 then 4, 5
    (include/adamvs_hip.h); lane l of fragment (k-step kc, patch row i, channel tile) holds cout = 16 tile + (l & 15), cin = 4 kc + (l >> 4)."""
    assert pk.dtype == torch.float32 and pk.numel() == 24 * D * D
    lo = pk[:16 * D * D].reshape(D // 4, 4, D // 16, 64, 4).double()
    hi = pk[16 * D * D:].reshape(D // 4, 4, D // 16, 64, 2).double()
    frag = torch.cat([lo, hi], dim=-1)                                       # [kc][i][tile][lane][j]
    u = torch.zeros(4, 6, D, D, dtype=F64)
    for lane in range(64):
        co16, k4 = lane & 15, lane >> 4
        u[:, :, co16::16, k4::4] = frag[:, :, :, lane, :].permute(1, 3, 2, 0)
    return u


def emulate(u, x, bias):
    """Y = At2 [ U .* (Bt2 d B4) ] A4 over the 2 x 4 tiles of x [cin][h][w] (zero outside the map; outputs past the edge dropped), the
    bias entering at position (1, 1) of the products as in the kernel."""
    D, h, w = x.shape
    th, tw = (h + 1) // 2, (w + 3) // 4
    xp = torch.zeros(D, 2 * th + 2, 4 * tw + 2, dtype=F64)
    xp[:, 1:h + 1, 1:w + 1] = x
    out = torch.zeros(D, 2 * th, 4 * tw, dtype=F64)
    for ty in range(th):
        for tx in range(tw):
            d = xp[:, 2 * ty:2 * ty + 4, 4 * tx:4 * tx + 6]
            v = torch.einsum("ik,ckl,jl->ijc", BT2, d, BT4)
            m = torch.einsum("ijoc,ijc->ijo", u, v)
            m[1, 1] += bias
            out[:, 2 * ty:2 * ty + 2, 4 * tx:4 * tx + 4] = torch.einsum("ai,ijo,bj->oab", AT2, m, AT4)
    return out[:, :h, :w]


@pytest.mark.parametrize("D", [64, 192])
def test_packed_fragments_evaluate_the_convolution(D):
    """From the PACKED array, in float64: unpack the fragment order, Bt d B, the products, At M A -- against conv2d in float64 to
    1e-12, on a map that is ragged in both directions.  The filters are multiples of 48 and the scales powers of two, so that
    U = G w G4^T (entries of 1/2 and 1/24) is exact in fp32 and the one rounding of the packing drops nothing; the inputs are small
    integers.  What is left is the matrices, the fragment order and the bias position."""
    g = torch.Generator().manual_seed(D)
    wt = 48.0 * torch.randint(-8, 9, (D, D, 3, 3), generator=g).to(F64)
    scale = 2.0 ** torch.randint(-1, 2, (D,), generator=g).to(F64)
    bias = torch.randint(-50, 51, (D,), generator=g).to(F64)
    h, w = 5, 7
    x = torch.randint(-4, 5, (D, h, w), generator=g).to(F64)
    u = unpack(packing.pack_reg_layer_wino24(wt.float(), scale.float()), D)
    exact = torch.einsum("ik,ockl,jl->ijoc", packing.WINO_G, wt * scale.reshape(-1, 1, 1, 1), packing.WINO_G4)
    assert float((u - exact).abs().max() / exact.abs().max()) < 1e-14       # the rounding to fp32 dropped nothing (1/6 in float64: 1e-16)
    ref = torch.nn.functional.conv2d(x[None], wt * scale.reshape(-1, 1, 1, 1), bias, padding=1)[0]
    got = emulate(u, x, bias)
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-12


def test_the_unit_element_at_1_1_reaches_every_output_of_the_tile():
    """The kernel starts accumulator position (1, 1) from the bias: At2 E A4 must be all ones for E = the unit element at (1, 1)."""
    e = torch.zeros(4, 6, dtype=F64)
    e[1, 1] = 1.0
    assert torch.equal(AT2 @ e @ AT4.T, torch.ones(2, 4, dtype=F64))


def test_random_filters_round_once():
    """U is formed in double precision and rounded to fp32 once: every packed value is the fp32 nearest to G w G4^T."""
    D = 64
    g = torch.Generator().manual_seed(1)
    wt, scale = torch.randn(D, D, 3, 3, generator=g), torch.rand(D, generator=g) + 0.5
    u = unpack(packing.pack_reg_layer_wino24(wt, scale), D)
    exact = torch.einsum("ik,ockl,jl->ijoc", packing.WINO_G, wt.double() * scale.double().reshape(-1, 1, 1, 1), packing.WINO_G4)
    assert torch.equal(u.float(), exact.float())


def test_the_blob_keeps_its_offsets_and_grows_at_the_end(monkeypatch):
    """pack_cost_reg_net_2d: the 11 direct blocks and the five F(2x2, 3x3) blocks are where they were (bench.py and the tests slice
    the blob there); conv0 and prob in the F(2x4, 3x3) form follow at the widths from 128 up; the library expects that length."""
    from ada_mvs_amd.models.adamvs import CostRegNet2D
    lib = _lib.load()
    for D in (64, 128):
        net = CostRegNet2D(D)
        sd = synth.seeded_state_dict(net, seed=3)
        blob = packing.pack_cost_reg_net_2d(sd, "")
        with monkeypatch.context() as mp:
            mp.setattr(packing, "WINO24_BLOB_WIDTHS", ())                    # the packing of before
            old = packing.pack_cost_reg_net_2d(sd, "")
        n_old = 11 * (9 * D * D + D) + 5 * 16 * D * D
        assert old.numel() == n_old and torch.equal(blob[:n_old], old)
        assert blob.numel() == lib.adamvs_cost_reg_net_2d_weight_floats(D, 0) == n_old + (2 * 24 * D * D if D >= 128 else 0)
        if D >= 128:
            for k, name in enumerate(("conv0", "prob")):
                if name == "prob":
                    w, scale = sd["prob.weight"], torch.ones(D)
                else:
                    bn = lambda s: sd["%s.bn.%s" % (name, s)].float()      # noqa: E731
                    w, scale = sd[name + ".conv.weight"], bn("weight") / torch.sqrt(bn("running_var") + packing.BN_EPS)
                assert torch.equal(blob[n_old + k * 24 * D * D:n_old + (k + 1) * 24 * D * D], packing.pack_reg_layer_wino24(w, scale)), name
        assert packing.pack_cost_reg_net_2d(sd, "", "bf16x3").numel() == 11 * (9 * D * D + D)
