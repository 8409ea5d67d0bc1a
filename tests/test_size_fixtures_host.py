"""The condition the size sweeps rest on (tests/size_fixtures.py), checked on the CPU: over every fixture run the oracle's
race margin stays at or above MIN_MARGIN, so the GPU tests may demand exact equality at every step."""
import numpy as np
import pytest

from tests.size_fixtures import (DM_NOISE_MODES, DM_RELOAD_CASE, DM_SEEDS, DM_SINGLE_CASES, DM_STEPS, DM_TEAM_CASES, MIN_MARGIN,
                                 RAW_BITS, RAW_NOISE_SEEDS, dm_distinct_bound, dm_fixture, raw_fixture)


def test_case_tables_cover_what_the_library_dispatches():
    assert DM_STEPS % 64 != 0
    assert {H // 64 for H, Q in DM_TEAM_CASES} == {8, 10, 12, 14}          # every dm_team_kernel<CPL>
    assert {H for H, Q in DM_TEAM_CASES if Q == 256} == {512, 640, 768, 896}
    assert {Q // 32 for H, Q in DM_TEAM_CASES} == {2, 4, 6, 8}             # every per-workgroup class count
    assert {(2, 2), (1024, 256)} <= set(DM_SINGLE_CASES)                    # the single kernel's limits
    assert set(DM_TEAM_CASES) & set(DM_SINGLE_CASES)                        # one size shared by both kernels
    assert set(DM_TEAM_CASES) | set(DM_SINGLE_CASES) == set(DM_SEEDS)
    assert all(phx >> 32 and phx & 0xFFFFFFFF for _, phx in DM_SEEDS.values())   # both Philox key words set
    assert set(RAW_NOISE_SEEDS) == {(b, r) for b in RAW_BITS for r in (2, 5)}


@pytest.mark.parametrize('noise', DM_NOISE_MODES)
@pytest.mark.parametrize('H,Q', sorted(DM_SEEDS))
def test_dm_fixture_has_no_near_tie(H, Q, noise):
    """Both builds of the oracle (the GPU tests use the fast one): the same trajectory, margin >= MIN_MARGIN at every step of
    both softmaxes, and enough distinct values that the GPU tests' collapsed-sampler check can pass."""
    fx = dm_fixture(H, Q, noise)
    plain = dm_fixture(H, Q, noise, False, False)
    print(f'({H},{Q}) {noise}: oracle min margin fast {fx["min_margin"]:.2e} plain {plain["min_margin"]:.2e}, '
          f'distinct coarse {len(np.unique(fx["coarse"]))} fine {len(np.unique(fx["fine"]))}')
    assert fx['margin'].shape == (DM_STEPS, 2)
    assert fx['min_margin'] >= MIN_MARGIN and plain['min_margin'] >= MIN_MARGIN
    np.testing.assert_array_equal(fx['coarse'], plain['coarse'])
    np.testing.assert_array_equal(fx['fine'], plain['fine'])
    assert len(np.unique(fx['coarse'])) > dm_distinct_bound(Q) and len(np.unique(fx['fine'])) > dm_distinct_bound(Q)
    assert fx['coarse'].min() >= 0 and fx['coarse'].max() < Q and fx['fine'].min() >= 0 and fx['fine'].max() < Q


def test_dm_reload_fixture_has_no_near_tie():
    H, Q = DM_RELOAD_CASE
    fx, before = dm_fixture(H, Q, 'injected', True), dm_fixture(H, Q, 'injected')
    print(f'({H},{Q}) reloaded: oracle min margin {fx["min_margin"]:.2e}')
    assert fx['min_margin'] >= MIN_MARGIN
    assert not np.array_equal(fx['coarse'], before['coarse'])
    assert len(np.unique(fx['coarse'])) > dm_distinct_bound(Q) and len(np.unique(fx['fine'])) > dm_distinct_bound(Q)


@pytest.mark.parametrize('bits,B', sorted(RAW_NOISE_SEEDS))
def test_raw_fixture_has_no_near_tie(bits, B):
    """Free run and teacher-forced pass of the oracle: margin >= MIN_MARGIN at every step of every row; forcing the oracle's
    own samples reproduces its free run; every class count really has more than one class in play."""
    fx = raw_fixture(bits, B)
    print(f'bits {bits} rows {B}: oracle min margin {fx["min_margin"]:.2e}, distinct labels {len(np.unique(fx["free"]["labels"]))}')
    assert fx['free']['labels'].shape == (fx['L'], B) and fx['forced']['logits'].shape == (fx['L'], B, 2 ** bits)
    assert fx['min_margin'] >= MIN_MARGIN
    np.testing.assert_array_equal(fx['forced']['labels'], fx['free']['labels'])
    assert fx['free']['labels'].min() >= 0 and fx['free']['labels'].max() < 2 ** bits
    assert len(np.unique(fx['free']['labels'])) > min(8, 2 ** bits / 2)
