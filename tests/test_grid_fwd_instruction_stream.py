"""k_grid_fwd_planes after its instruction diet (DESIGN.md "The forward kernel's instruction stream"): the PLAIN instantiation -- Linear
interpolation, a prime hash, 2-D, two features per level, hit lists -- and the generic body that serves everything else, bit for bit against
two things the diet does not touch: the CPU oracle and the Rows kernel k_grid_fwd (TCNN_AMD_GRID_ROWS_PLANES=0).

What is compared.  An Encoding module's forward pass with parameter gradients runs k_grid_fwd_planes + k_planes_to_rows and, with
TCNN_AMD_SCATTER_LISTS=1 (the switch the list tests of test_gpu_parity.py use to get lists at small batches), records hit lists; its
backward pass feeds them to k_grid_scatter_lists.
  * The level planes: the encoded matrix, every element, against the oracle's (grid.h:58-213) and the Rows kernel's.
  * The hit lists -- elements (both entries, both half weights), sample numbers, heads, stragglers: the library hands no list to the host,
    so they are compared through what they determine.  The list-fed kernel sums, per table entry, the products weight x dL/dy of exactly the
    elements (and stragglers) that name the entry, as exact integers, and rounds once: with a random dL/dy the result equals the oracle's
    exact scatter (grid.h:215-320, one final rounding) bit for bit only if every element names the right entries with the right weights
    for the right sample, every head cuts the runs at the right place and every straggler is there exactly once.  The order inside a
    run (ranks come from LDS atomics) does not enter an exact sum.  list_scatters() asserts that this kernel is the one that ran.
  * Grids that never record lists (Rng hash) are compared the same way through the bit planes.

Which body a case runs (grid_planes_plain, tcnn_common.h): Linear with Prime / CoherentPrime / ReversedPrime in 2-D with lists: PLAIN, its
hashed body on the levels whose cells exceed the table, its dense body on the others; Nearest, Smoothstep, Rng and 3-D: the generic body.

Shapes: the smallest at which each branch exists.  GRID_2D (L = 8, base 4, scale 2, T = 2^14; the issue's grid): dense levels of one
chunk (0 .. 4), and a dense (5) and two hashed levels (6, 7) of 16384 entries in two chunks of 8192 -- on the hashed ones every other row
with odd x has its corner B in the other chunk, so the straggler path runs thousands of times.  GRID_2D_ODD (L = 7, base 12, T = 2^17) is
the smallest grid whose levels are cut finely (grid_scatter_setup_levels cuts into up to 64 chunks of at least 256 entries once a level
exceeds 8 x 8192 entries): level 3 (96 x 96) has 36 chunks of 256 with edges inside the rows of cells, level 4 (192 x 192 = 36864) has 64
chunks of 576 -- no power of two: the division --, levels 5 and 6 are hashed into 64 chunks of 2048.
n = 1024 and 4096: whole items (1024 samples); 1280: one wave's 256 samples behind a whole item, the item's other three waves past the end; 65536 + 256: the default list threshold of 2-D grids and a
ragged item behind it.  (A module takes batches that are multiples of the batch granularity, 256 -- one wave of this kernel -- only, so no
smaller raggedness reaches the kernel.)
Inputs: coordinates exactly 0 and just below 1; one sample in every cell of a dense level's lattice (rows of cells, cx = 0 .. res - 1): every
pair of neighbouring entries of a lattice row is some sample's cell row, so even and odd x both occur (pair load, own load) and every
chunk edge inside such a row is straddled (the straggler path), whatever the level's scatter_per_chunk is.
"""
import numpy as np
import pytest

from conftest import CONFIG_C3A
from test_gpu_parity import _bits, _t
from test_list_gradients_in_mlp import R32, _exact_steps

pytestmark = pytest.mark.gpu

GRID_2D = {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 14, "base_resolution": 4, "per_level_scale": 2.0}
GRID_2D_ODD = {**GRID_2D, "n_levels": 7, "base_resolution": 12, "log2_hashmap_size": 17}
GRID_3D = {"otype": "HashGrid", "n_levels": 6, "n_features_per_level": 2, "log2_hashmap_size": 14, "base_resolution": 4, "per_level_scale": 2.0}
HASHES = ["Prime", "CoherentPrime", "ReversedPrime", "Rng"]

CASES = [(f"2d_{interp}_{h}_4096", 2, {**GRID_2D, "interpolation": interp, "hash": h}, 4096, 4) for interp in ("Nearest", "Linear", "Smoothstep") for h in HASHES]
CASES += [(f"2d_Linear_{n}", 2, GRID_2D, n, 4) for n in (1024, 1280, 65536 + 256)]
CASES += [(f"2d_{interp}_1280", 2, {**GRID_2D, "interpolation": interp}, 1280, 4) for interp in ("Nearest", "Smoothstep")]
CASES += [(f"2d_odd_chunks_{n}", 2, GRID_2D_ODD, n, lattice) for n, lattice in ((1280, 3), (4096, 4))]
CASES += [(f"3d_{n}", 3, GRID_3D, n, 2) for n in (512, 2048)]


def _inputs(oracle, n_in, enc_cfg, n, lattice_level):
    x = oracle.Pcg32(42).uniform_strided(n * n_in).reshape(n, n_in)
    below_one = np.nextafter(np.float32(1.0), np.float32(0.0))
    x[:8] = np.float32([[0.0] * n_in, [below_one] * n_in, [0.0] + [below_one] * (n_in - 1), [below_one] + [0.0] * (n_in - 1), [0.5] * n_in, [1e-7] * n_in, [0.25] * n_in, [0.75] * n_in])
    # the lattice of level `lattice_level` (scale = base 2^level - 1, pos = x scale + 0.5: x = c / scale lies in the middle of cell c), whole
    # rows of cells, as many as half the batch holds, spread so that their numbers take every residue of a chunk's rows
    res = enc_cfg["base_resolution"] * 2 ** lattice_level
    rows = min(res, (n // 2) // res)
    cx, cy = np.meshgrid(np.arange(res), (np.arange(rows) * (res // rows + 1)) % res)
    pts = np.stack([cx.ravel(), cy.ravel()] + [cy.ravel()] * (n_in - 2), axis=1).astype(np.float32) / np.float32(res - 1)
    x[8:8 + len(pts)] = pts
    return x


@pytest.mark.parametrize("name,n_in,enc_cfg,n,lattice_level", CASES, ids=[c[0] for c in CASES])
def test_planes_and_lists_match_oracle_and_rows_kernel(tcnn, oracle, monkeypatch, name, n_in, enc_cfg, n, lattice_level):
    """Module docstring: the encoded matrix and the exact gradient of a random dL/dy, from the plane kernel with hit lists, against the
    oracle and against the Rows kernel with the bit-plane scatter."""
    ref = oracle.create_encoding(n_in, enc_cfg, alignment=0)
    params_h = oracle.half_bits(oracle.Pcg32(3).uniform_strided(ref.n_params, -1.0, 1.0))
    x = _inputs(oracle, n_in, enc_cfg, n, lattice_level)
    width = ref.padded_output_width
    dy = oracle.half_bits(oracle.Pcg32(9).uniform_strided(n * width, -2.0, 2.0).reshape(n, width))
    dy[::7] = 0
    want_out, _ = ref.forward(x, params_h)
    want_g = np.zeros(ref.n_params, dtype=np.uint16)
    ref.backward_exact(x, dy, want_g)
    assert np.count_nonzero(want_g) > 100

    def run(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        native = tcnn.Encoding(n_in, enc_cfg).native_tcnn_module
        xt, pt = _t(x), _t(params_h.view(np.float16)).requires_grad_(True)
        ctx, out = native.fwd(xt, pt)
        _, g = native.bwd(ctx, xt, pt, out, _t(dy.view(np.float16)))
        res = _bits(out).copy().reshape(n, width), _bits(g).copy(), native.list_scatters()
        for k in env:
            monkeypatch.delenv(k)
        return res

    out, g, n_lists = run({"TCNN_AMD_SCATTER_LISTS": "1"})
    assert n_lists == (0 if enc_cfg.get("hash") == "Rng" else 1), "the list-fed gradient kernel is the one under test (Rng grids record no lists)"
    assert np.array_equal(out, want_out), f"{np.count_nonzero(out != want_out)} elements of the planes differ from the oracle's"
    assert np.array_equal(g, want_g), f"{np.count_nonzero(g != want_g)} gradient elements differ from the oracle's exact scatter"
    out_rows, g_rows, n_lists_rows = run({"TCNN_AMD_GRID_ROWS_PLANES": "0", "TCNN_AMD_SCATTER_LISTS": "0"})
    assert n_lists_rows == 0
    assert np.array_equal(out, out_rows) and np.array_equal(g, g_rows)


def test_three_steps_of_the_flagship_match_oracle(tcnn, oracle, monkeypatch):
    """BASELINE config 3a at n = 2^16 (the smallest batch at which its lists are the default), three training_step()s on three seeded
    batches through the fused MLP kernel: the network's output bits and dL/doutput bits are the oracle's (asserted inside _exact_steps) and the
    grid's gradient is the oracle's exact scatter bit for bit after every step -- Overwrite, then Accumulate twice, so the third comparison
    carries all three forward passes.  (Bit-exactness against the oracle exists for gradients, as in tests/test_list_gradients_in_mlp.py;
    the parameters after Adam are compared within tolerances by the existing parity tests and are not restated here.)"""
    from tinycudann.native import GRADIENT_ACCUMULATE, GRADIENT_OVERWRITE

    for k, v in R32.items():
        monkeypatch.setenv(k, v)
    steps = 0
    for tr, got, want in _exact_steps(tcnn, oracle, CONFIG_C3A, 2, 1 << 16, (GRADIENT_OVERWRITE, GRADIENT_ACCUMULATE, GRADIENT_ACCUMULATE)):
        steps += 1
        assert tr.list_scatters() == steps, "the hit lists are the default at this batch size"
        assert np.count_nonzero(want) > 100_000
        assert np.array_equal(got, want), f"step {steps}: {np.count_nonzero(got != want)} gradient elements differ"
    assert steps == 3
