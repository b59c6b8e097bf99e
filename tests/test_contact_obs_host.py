"""CPU tests (-m "not gpu") of the whole-batch contact observations: the C boundary (header, binding) and the independent numpy
restatement of the body rows (tests/numpy_contacts.py) on a hand-written contact list."""
import os
import re

import numpy as np

from real_robots_amd import _native as nat
from tests import numpy_contacts as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, 'include', 'realrobot.h')).read()


def test_header_declares_the_call_and_the_three_fields_in_abi_7():
    h = _header()
    assert re.search(r'\bint\s+rr_contact_observations\s*\(\s*rr_env\s*\*\s*env\s*\)\s*;', h)
    fields = dict((k, int(v)) for k, v in re.findall(r'\b(RR_F_[A-Z_]+)\s*=\s*(\d+)', h))
    assert (fields['RR_F_CONTACTS'], fields['RR_F_BODY_FORCE'], fields['RR_F_BODY_PARTNERS'], fields['RR_F_COUNT']) == (13, 14, 15, 16)
    assert (nat.F_CONTACTS, nat.F_BODY_FORCE, nat.F_BODY_PARTNERS) == (13, 14, 15)
    assert int(re.search(r'#define\s+RR_CONTACT_ROWS\s+(\d+)', h).group(1)) == nat.CONTACT_ROWS == 20 == len(nat.LINK_NAMES) + 3
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION == 7
    doc = h[h.index('int rr_get_contacts('):h.index('int rr_contact_observations(')]
    assert 'robot.py:131-150' in doc and 'Out of scope' in doc and 'STREAM CONTRACT' in doc


def test_binding_lists_and_loads_the_symbol():
    assert 'rr_contact_observations' in nat.SYMBOLS
    L = nat.load_library()
    assert L.rr_contact_observations.restype is not None and len(L.rr_contact_observations.argtypes) == 1
    assert L.rr_abi_version() == 7


def _row(a, b, link, dist, force):
    return [a, b, link, 0.1, 0.2, 0.3, 0.0, 0.0, 1.0, dist, force, 0.5]


def test_numpy_body_rows_on_a_hand_written_list():
    """Five contacts: skin_00 x object 0 twice, a link x the table, object 0 x object 1, and one at distance 0.15 that the
    0.1 threshold (robot.py:136) drops."""
    skin_00, skin_10, link_4 = nat.LINK_NAMES.index('skin_00'), nat.LINK_NAMES.index('skin_10'), nat.LINK_NAMES.index('lbr_iiwa_link_4')
    contacts = np.array([_row(8, 16, skin_00, -0.001, 3.5), _row(8, 16, skin_00, 0.005, 1.25), _row(3, -1, link_4, 0.0, 10.0),
                         _row(16, 17, -1, 0.01, 0.75), _row(10, -1, skin_10, 0.15, 99.0)], np.float32)
    force, partners = nc.body_rows([contacts, np.zeros((0, 12), np.float32)])
    assert force.shape == (2, 20, 2) and force.dtype == np.float32 and partners.shape == (2, 20) and partners.dtype == np.uint32
    exp_f, exp_p = np.zeros((20, 2), np.float32), np.zeros(20, np.uint32)
    exp_f[skin_00], exp_p[skin_00] = (3.5, 4.75), 0b00010            # touches object 0
    exp_f[link_4], exp_p[link_4] = (10.0, 10.0), 0b00001             # touches a static body
    exp_f[17], exp_p[17] = (3.5, 5.5), 0b10100                       # object 0: the robot (twice) and object 1
    exp_f[18], exp_p[18] = (0.75, 0.75), 0b00010                     # object 1: object 0
    assert (force[0] == exp_f).all() and (partners[0] == exp_p).all()
    assert not force[1].any() and not partners[1].any()
    # the sum is a sequential float32 loop in contact order: 2^24 + 1 + 1 stays 2^24 (a pairwise sum would give 2^24 + 2)
    big = np.array([_row(16, -1, -1, 0.0, 16777216.0), _row(16, -1, -1, 0.0, 1.0), _row(16, -1, -1, 0.0, 1.0)], np.float32)
    f, p = nc.body_rows([big])
    assert f[0, 17, 1] == np.float32(16777216.0) and f[0, 17, 0] == np.float32(16777216.0) and p[0, 17] == 1
    f, _ = nc.body_rows([big[::-1]])
    assert f[0, 17, 1] == np.float32(16777218.0)
