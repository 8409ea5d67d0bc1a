"""CPU: `wrnn_train_teamg_plan`, the host-only layout of persistent XCD-team GRU recurrences for a run-time rnn_dims
(csrc/train_teamg_plan.h), and the declaration / export / binding of it and of `wrnn_train_last_recurrence`.  The plan is the
authority on which rnn_dims such kernels can take: a workgroup's slice of W_hh must fit 160 KiB of LDS, there is no streaming."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('wrnn_train_last_recurrence', 'wrnn_train_teamg_plan')
OK, INVALID, UNSUPPORTED = 0, -1, -7
LDS_LIMIT = 160 * 1024


def test_the_entry_points_are_declared_exported_and_bound():
    from tacotronv2_wavernn_chinese_amd import _cabi
    hdr = open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read()
    declared = set(re.findall(r'\b(wrnn_[a-z_]+)\s*\(', hdr))
    lib = _cabi.load_library()
    for s in SYMBOLS:
        assert s in declared, s
        assert s in _cabi.EXPORTED_SYMBOLS, s
        assert getattr(lib, s).argtypes is not None, s          # bound: load_library() gave it a signature
    for name, value in (('WRNN_TRAIN_RAN_STEPS', 0), ('WRNN_TRAIN_RAN_TEAM512', 1), ('WRNN_ABI_VERSION', 9)):
        assert re.search(rf'#define {name} {value}\b', hdr), name
    assert hasattr(_cabi.NativeVocoder, 'train_last_recurrence')
    assert lib.wrnn_train_last_recurrence(None, None, None) == INVALID


def test_plan_units_lds_and_the_limit():
    from tacotronv2_wavernn_chinese_amd._cabi import train_teamg_plan
    prev = {4: (0, 0), 8: (0, 0)}
    admitted = {4: [], 8: []}
    for H in range(16, 1025, 16):
        per_rows = {}
        for rows in (4, 8):
            p = train_teamg_plan(H, rows)
            assert p['status'] in (OK, UNSUPPORTED), (H, rows, p)
            assert p['units_per_wg'] == -(-H // 32), (H, rows, p)
            assert p['lds_fwd'] > 0 and p['lds_bwd'] > 0 and p['mail_granules'] > 0, (H, rows, p)
            assert p['lds_fwd'] >= prev[rows][0] and p['lds_bwd'] >= prev[rows][1], (H, rows, p, prev[rows])    # non-decreasing in H
            prev[rows] = (p['lds_fwd'], p['lds_bwd'])
            assert (p['status'] == OK) == (p['lds_fwd'] <= LDS_LIMIT and p['lds_bwd'] <= LDS_LIMIT), (H, rows, p)
            if p['status'] == OK:
                admitted[rows].append(H)
            per_rows[rows] = p
        assert per_rows[8]['lds_fwd'] >= per_rows[4]['lds_fwd'] and per_rows[8]['lds_bwd'] >= per_rows[4]['lds_bwd'], H   # ... and in rows
        assert per_rows[8]['mail_granules'] >= per_rows[4]['mail_granules'], H
    assert 512 in admitted[8] and 256 in admitted[8] and 16 in admitted[8]
    assert train_teamg_plan(1024, 8)['status'] == UNSUPPORTED and train_teamg_plan(1024, 4)['status'] == UNSUPPORTED
    # the admitted dims are a prefix: nothing above the limit comes back in
    for rows in (4, 8):
        assert admitted[rows] == list(range(16, admitted[rows][-1] + 1, 16)), rows
    assert set(admitted[8]) <= set(admitted[4])
    # rows 1..4 are the 4-row instantiation, 5..8 the 8-row one
    for H in (16, 272, 512):
        assert all(train_teamg_plan(H, r) == train_teamg_plan(H, 4) for r in (1, 2, 3))
        assert all(train_teamg_plan(H, r) == train_teamg_plan(H, 8) for r in (5, 6, 7))


def test_plan_at_512_is_the_layout_of_the_512_kernels():
    """U = 16 and a 96 KiB image next to R x 512 floats of h: what csrc/train_team.hip has compiled in (FL<NQ>::L_H = 24576 floats)."""
    from tacotronv2_wavernn_chinese_amd._cabi import train_teamg_plan
    for rows, R in ((4, 4), (8, 8)):
        p = train_teamg_plan(512, rows)
        assert p['units_per_wg'] == 16
        assert p['lds_fwd'] == 4 * (24576 + R * 512 + 16)
        assert p['mail_granules'] == 2 * 32 * R * 32 * 16      # BL<NQ>::MAIL


@pytest.mark.parametrize('H,rows', [(100, 8), (0, 8), (8, 4), (-16, 4), (512, 0), (512, 9), (512, -1)])
def test_plan_refuses_bad_arguments(H, rows):
    from tacotronv2_wavernn_chinese_amd._cabi import train_teamg_plan
    p = train_teamg_plan(H, rows)
    assert p['status'] == INVALID and p['units_per_wg'] == 0 and p['lds_fwd'] == 0


def test_plan_accepts_null_outputs():
    from tacotronv2_wavernn_chinese_amd import _cabi
    lib = _cabi.load_library()
    assert lib.wrnn_train_teamg_plan(256, 8, None, None, None, None) == OK
    assert lib.wrnn_train_teamg_plan(1024, 8, None, None, None, None) == UNSUPPORTED
