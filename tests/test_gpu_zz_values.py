"""GPU: every f64, integer and string edge of tests/_values.py rendered by the gfx950 build at every site the renderer writes a
scalar from, byte for byte against the plain Python expectation and the oracle (tests/_value_sites.py; the same functions run on the
kernel-logic harness in tests/test_values.py).  What only the device shows: how hipcc lowers the 128-bit shifts and compares of the
two-register digit generator, generic pointers into the LDS bignum workspace, one lane working between two block barriers.

Each site is ONE batch in ONE child process under a time limit, and nothing is run again after a failure.  Measured on an MI355X,
seconds inside the child (documents built + device + oracle): strings 0.15, map 0.48, fused 0.47, nested 0.34, movable 0.37; a whole
child process, interpreter start and runtime initialisation included, about 0.7 s; the slowest whole test, the list site with the
entire corpus rendered twice, 1.24 s — richtext and snapshot finished below that.  The limit of every site is 5 s: three times the
slowest, rounded up."""
import json, os, subprocess, sys

import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT = dict.fromkeys(("list", "map", "nested", "movable", "richtext", "snapshot", "fused", "strings"), 5)


def _site(name):
    try:
        p = subprocess.run([sys.executable, os.path.join(_HERE, "_value_sites.py"), name], cwd=os.path.dirname(_HERE), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=LIMIT[name])
    except subprocess.TimeoutExpired as e:
        pytest.fail("site %s did not finish within %d s\n%s" % (name, LIMIT[name], (e.stderr or b"").decode(errors="replace")[-4000:]))
    assert p.returncode == 0, "site %s: exit status %d\n%s" % (name, p.returncode, p.stderr.decode(errors="replace")[-6000:])
    out = json.loads(p.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(out))
    return out


def test_list_items_the_whole_f64_corpus():
    out = _site("list")
    assert out["doubles"] >= 45000 and out["slab_overflow_documents"] > 0 and out["forced_exact_size_documents"] == out["documents"]


def test_map_entry_values_and_the_three_integer_formatters():
    out = _site("map")
    assert out["doubles"] >= 5000 and out["integers"] >= 150


def test_nested_values():
    assert _site("nested")["doubles"] >= 2000


def test_movable_list_insert_and_set():
    assert _site("movable")["doubles"] >= 2000


def test_richtext_attribute_values():
    assert _site("richtext")["doubles"] >= 1500


def test_snapshot_state_path():
    out = _site("snapshot")
    assert out["state_documents"] == out["documents"] >= 50


def test_folded_map_path():
    out = _site("fused")
    assert out["fused_documents"] == out["documents"] and out["doubles"] >= 5000


def test_strings():
    assert _site("strings")["strings"] >= 300
