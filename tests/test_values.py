"""Scalar rendering on the CPU: the plain references of tests/_values.py against the oracle on the whole corpus, the host build
of f64_json (lm_f64.h) against them on the whole corpus, and every rendering site of tests/_value_sites.py through the kernel-logic
harness on thinned corpora — so that a failure of tests/test_gpu_zz_values.py on the device separates "logic" from "gfx950 build"."""
import collections, ctypes, json

import pytest

import _emu, _oracle
import _values as V
import _value_sites as sites
from loro_amd._cabi import Context


def _harness():
    return Context(_emu.binding())


def test_corpora_hold_what_they_promise():
    c = V.f64_corpus()
    assert 45000 <= len(c) <= 53000 and len(set(c)) == len(c) and c == V.f64_corpus()
    kinds = collections.Counter(V.f64_generator(b) for b in c)
    assert kinds["u128"] >= 10000 and kinds["big"] >= 10000 and kinds["int"] >= 400 and kinds["zero"] == 2 and kinds["null"] >= 8, kinds
    finite = [b for b in c if V.f64_generator(b) not in ("null", "zero")]
    assert {V.f64_scale(b) for b in finite} == set(range(-1074, 1024))          # every input of the decimal-exponent estimate
    assert {(b >> 52) & 0x7FF for b in c} == set(range(2048))
    digits = collections.Counter(len(V.ryu_layout(V.f64_of(b)).strip("-").split("e")[0].replace(".", "").strip("0")) for b in finite)
    assert all(digits[n] >= 100 for n in range(1, 18)), digits
    ints = {len(V.ryu_layout(V.f64_of(b))) - 2 for b in c if V.f64_generator(b) == "int" and not b >> 63}
    assert ints == set(range(1, 17))                                            # "<n>.0" at every digit count
    for e2 in list(range(-123, -118)) + list(range(58, 63)):
        assert sum(1 for b in c if (b >> 52) & 0x7FF == e2 + 1075) >= 30
    i = V.i64_corpus()
    assert 150 <= len(i) <= 170 and len(set(i)) == len(i) and 2 ** 63 - 1 in i and -(2 ** 63) in i
    assert all(s * v in i for k in range(19) for v in (10 ** k, 10 ** k - 1, 10 ** k + 1) for s in (1, -1))
    s = V.str_corpus()
    assert len(set(s)) == len(s) and {len(x) for x in s} >= {0, 1, 63, 64, 65, 127, 128, 129, 200}
    assert all(chr(b) in s for b in range(0x80)) and {len(x.encode()) <= 24 for x in s} == {True, False}
    assert {len(x.encode()) for x in s} >= {24, 25}


def test_known_layouts():
    for x, want in [(1.5, "1.5"), (0.0, "0.0"), (-0.0, "-0.0"), (100.0, "100.0"), (0.1, "0.1"), (1e16, "1e16"), (1e15, "1000000000000000.0"),
                    (123456789012345680.0, "1.2345678901234568e17"), (1e-5, "0.00001"), (1e-6, "1e-6"), (5e-324, "5e-324"),
                    (1.7976931348623157e308, "1.7976931348623157e308"), (-2.5e-3, "-0.0025"), (9007199254740993.0, "9007199254740992.0"),
                    (float("inf"), "null"), (float("nan"), "null"), (1e21, "1e21"), (2 / 3, "0.6666666666666666")]:
        assert V.ryu_layout(x) == want


def test_the_plain_reference_equals_the_oracle_on_the_whole_corpus():
    o = _oracle.lib()
    o.lo_json_f64.restype = ctypes.c_int
    o.lo_json_f64.argtypes = [ctypes.c_double, ctypes.c_char_p]
    buf = ctypes.create_string_buffer(64)
    for bits in V.f64_corpus():
        n = o.lo_json_f64(V.f64_of(bits), buf)
        assert buf.raw[:n].decode() == V.ryu_layout(V.f64_of(bits)), hex(bits)


def test_the_host_build_of_f64_json_equals_the_plain_reference_on_the_whole_corpus():
    e = _emu.binding().lib
    e.lmemu_f64_json.restype = ctypes.c_int
    e.lmemu_f64_json.argtypes = [ctypes.c_uint64, ctypes.c_char_p]
    buf = ctypes.create_string_buffer(64)
    for bits in V.f64_corpus():
        n = e.lmemu_f64_json(bits, buf)
        assert 0 < n <= 32 and buf.raw[:n].decode() == V.ryu_layout(V.f64_of(bits)), (hex(bits), buf.raw[:n])


def test_the_decimal_exponent_estimate_has_room_for_any_rounding():
    """lm_f64.h computes ceil(n · log10 2 - 1e-10) in double, n = e2 + bitlen - 1: for every n the product is far enough from an
    integer that neither the 1e-10, nor the rounding of the product, nor a fused multiply-add can move the result — checked here
    in exact integer arithmetic: 10^(est-1) < 2^n <= 10^est … (2^n is never a power of ten for n != 0)"""
    for n in range(-1074, 1024):
        t = float(n) * 0.30102999566398120
        est = int(t)
        if float(est) < t - 1e-10:
            est += 1
        if t < 0 and float(est) > t + 1.0:
            est -= 1
        if n >= 0:
            assert 10 ** est >= 2 ** n and (est == 0 or 10 ** (est - 1) < 2 ** n), n
        else:
            assert est <= 0 and 10 ** -est <= 2 ** -n < 10 ** (1 - est), n
        assert n == 0 or abs(t - round(t)) > 4.5e-4, (n, t)       # room: the double product is within 1e-13 of n · log10 2


def test_wave_primitives_selftest_in_the_harness():
    with _harness() as c:
        assert c.b.selftest(c.h) == 0


@pytest.mark.parametrize("site", list(sites.SITES))
def test_site(site):
    out = sites.SITES[site](_harness, False)
    print(json.dumps(out))
