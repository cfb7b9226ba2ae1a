"""The designed operands of tests/test_gpu_first_layer_exact.py, proved on the CPU (tests/_first_exact.py): every design x case has
its exactness proof, populates the last term of its split and gives an fp32-representable float64 reference; and the inputs
DISCRIMINATE: an emulated route (the split, then fp32 accumulation of every term in a shuffled order) matches the reference bit
for bit, and each of three mutations of that emulation — the last term dropped, the last term doubled, one tap read one pixel
off — changes fp32 values and flips threshold bits under the very bias / BatchNorm sets the GPU cases use."""
import pytest
import torch

import _first_exact as FE
import _grad_exact as G

PAIRS = [(g, d) for g in FE.GROUPS for d in g.designs]


def test_every_rung_form_and_split_of_the_table_has_a_group():
    have = {(g.rung, f, g.table_split) for g in FE.GROUPS for f in g.forms}
    missing = [t for t in FE.table() if t not in have]
    assert not missing, missing
    for g in FE.GROUPS:
        assert set(g.forms) <= set(FE.FORMS[g.rung]) and g.table_split in FE.SPLITS[g.rung], g.id
        assert max(g.geom[6:]) <= 35 and g.batch <= 3, g.id
        assert g.designs, g.id


def test_every_design_runs_on_every_rung_and_split():
    for rung, splits in FE.SPLITS.items():
        for split in splits:
            have = {d for g in FE.GROUPS if g.rung == rung and g.table_split == split for d in g.designs}
            assert have == set(FE.DESIGNS), (rung, split, have)


def test_dense_is_left_out_only_where_the_bound_keeps_it_from_the_last_term():
    """(the rule counts every weight as +-1: K elements of NEED_BITS + 2 bits must fit under 2^24 units)"""
    for g in FE.GROUPS:
        assert ("dense" in g.designs) == FE.dense_reaches(FE.K_of(g.geom), g.split) or g.kind == "xnor", g.id


@pytest.mark.parametrize("g,design", PAIRS, ids=[f"{g.id}-{d}" for g, d in PAIRS])
def test_design_is_proved_exact_and_populates_the_last_term(g, design):
    c = g.case(design)
    assert c.ok, c.why
    assert c.coverage >= FE.COVERAGE, c.coverage
    assert torch.equal(c.y32.to(torch.float64), c.y64)
    x = c.x
    assert bool(((x == 0) & ~torch.signbit(x)).any()) and bool(((x == 0) & torch.signbit(x)).any()), "+0 and -0"
    if g.batch >= 2:
        assert not bool(x[-1].any())
    if g.batch >= 3 and g.geom[6] > 31:
        assert not bool(x[-2, :, 31:].any()) and bool(x[-2, :, :31].any()) and bool(x[0, :, 31:].any())
    assert bool((c.bias == 0).any()) and bool((c.bias != 0).any())
    if g.kind == "xnor":
        assert G.quantum_exp(c.wq) is not None and torch.equal(c.wq, c.w)


def test_ramp_gives_neighbouring_tiles_and_channels_different_magnitudes():
    g = next(g for g in FE.GROUPS if g.rung == "first3x3" and g.geom[6:] == (33, 35))
    x = g.case("ramp").x[0].abs()
    top, bottom = float(x[:, :31].max()), float(x[:, 32:].max())
    left, right = float(x[:, :, :31].max()), float(x[:, :, 32:].max())
    assert bottom >= 2 * float(x[:, :8].max()) and right >= 2 * float(x[:, :, :8].max()), (top, bottom, left, right)
    per_channel = x.reshape(x.shape[0], -1).max(1).values
    assert float(per_channel.max()) >= 2 * float(per_channel.min())


def _emulated(g):
    """The groups whose emulation the mutation tests run: one per (rung, split), the smallest K first (the loop is K x terms long)."""
    seen, out = set(), []
    for grp in sorted(g, key=lambda t: FE.K_of(t.geom) * t.batch * t.geom[6] * t.geom[7]):
        if (grp.rung, grp.split) not in seen and min(FE.out_hw(grp.geom[6], grp.geom[7], *FE._pair(grp.geom[2]), *grp.geom[3:6])) >= 2:
            seen.add((grp.rung, grp.split))
            out.append(grp)
    return out


EMU = [(g, d) for g in _emulated(FE.GROUPS) for d in FE.DESIGNS if d in g.designs]
# the AlexNet geometry (K = 363) as well: the one where a dense image cannot populate the third bf16 term
EMU += [(g, d) for g in FE.GROUPS if g.rung == "s2d" and FE.K_of(g.geom) == 363 and g.batch == 2 and g.storage == "cl"
        and g.entry == "forward" and g.q == FE.QUANTA[0] for d in g.designs]


@pytest.mark.parametrize("g,design", EMU, ids=[f"{g.id}-{d}" for g, d in EMU])
def test_emulated_route_matches_and_every_mutation_is_caught(g, design):
    c = g.case(design)
    seed = FE.seed_of("emu", g.id, design)
    got = FE.emulate(c, seed)
    assert torch.equal(got.view(torch.int32), c.y32.view(torch.int32)), G.mismatch_report(got, c.y32, names=("n", "c", "y", "x"))
    sets = {"affine": FE.affine_set(c, seed), "batchnorm": FE.fold_bn(*FE.bn_set(c, seed))}
    want = {}
    for name, (alpha, beta) in sets.items():
        want[name] = FE.want_bits(c, alpha, beta)[0]
        assert torch.equal(FE.emulated_bits(got, alpha, beta), want[name]), name
        tie = FE.want_bits(c, alpha, beta)[1] == 0
        assert int(tie[..., 8:].sum()) >= 1, f"{name}: no accumulator sits exactly on its threshold"
    for mutation in FE.MUTATIONS:
        bad = FE.emulate(c, seed, mutate=mutation)
        diff = int((bad.view(torch.int32) != c.y32.view(torch.int32)).sum())
        assert diff > 0, f"{mutation}: the fp32 result does not change"
        for name, (alpha, beta) in sets.items():
            flips = int((FE.emulated_bits(bad, alpha, beta) != want[name]).sum())
            assert flips > 0, f"{mutation}: no threshold bit of the {name} set flips ({diff} fp32 values differ)"


LIN = FE.linear_cases()


@pytest.mark.parametrize("M,N,K,split,design,with_bias", LIN, ids=["-".join(str(v) for v in t) for t in LIN])
def test_linear_design_is_proved_exact(M, N, K, split, design, with_bias):
    c = FE.linear_case(M, N, K, split, design, with_bias)
    assert c.ok, c.why
    if design == "ramp" or FE.dense_reaches(K, split):
        assert c.coverage >= FE.COVERAGE, c.coverage
    if design == "ramp":
        rows = c.x.abs().max(1).values
        assert float(rows.max()) >= 2 * float(rows[rows > 0].min())
