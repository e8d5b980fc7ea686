"""README.md's table of environment switches against the names the code reads: every SHN_* name the product reads is in the
table, and every name in the table is read by the product or set by a test or a tool.  Reads files only."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LITERAL = re.compile(r'''["'](SHN_[A-Z0-9_]+)["']''')
DOCUMENTED = re.compile(r"`(SHN_[A-Z0-9_]+)[^`]*`")


def _text(path):
    with open(path, errors="replace") as f:
        return f.read()


def _product_files():
    files = glob.glob(os.path.join(ROOT, "shannon_amd", "**", "*.py"), recursive=True)
    files += [p for p in glob.glob(os.path.join(ROOT, "shannon_amd", "csrc", "*")) if os.path.isfile(p)]
    files += [os.path.join(ROOT, "shannon.py"), os.path.join(ROOT, "bench.py")]
    return files


def _read_by_product():
    names = set()
    for p in _product_files():
        names.update(LITERAL.findall(_text(p)))
    return names


def _documented():
    readme = _text(os.path.join(ROOT, "README.md"))
    start = readme.index("Environment switches (")
    table = [ln for ln in readme[start:].split("\n\n", 2)[1].splitlines() if ln.startswith("|")]
    assert len(table) > 3, "README.md: the switch table was not found under 'Environment switches'"
    return set(DOCUMENTED.findall("\n".join(table)))


def _set_by_tests_or_tools():
    text = []
    for d in ("tests", "tools"):
        for p in glob.glob(os.path.join(ROOT, d, "**", "*"), recursive=True):
            if os.path.isfile(p) and os.path.splitext(p)[1] in (".py", ".sh"):
                text.append(_text(p))
    return set(re.findall(r"\bSHN_[A-Z0-9_]+", "\n".join(text)))


def _covers(literal, names):
    """a literal that ends in _ is a prefix names are built from"""
    return any(n.startswith(literal) for n in names) if literal.endswith("_") else literal in names


def test_every_switch_the_product_reads_is_documented():
    documented = _documented()
    missing = sorted(n for n in _read_by_product() if not _covers(n, documented))
    assert not missing, "read by the code, not in README.md's switch table: %s" % missing


def test_every_documented_switch_is_read_or_set_somewhere():
    product = _read_by_product()
    prefixes = [n for n in product if n.endswith("_")]
    used = product | _set_by_tests_or_tools()
    stale = sorted(n for n in _documented() if n not in used and not any(n.startswith(p) for p in prefixes))
    assert not stale, "in README.md's switch table, read or set nowhere: %s" % stale


def test_the_table_holds_the_switches():
    # the parser itself: a table that lost its names (or a pattern that no longer matches) must not pass for "nothing stale"
    documented = _documented()
    assert len(documented) > 80 and {"SHN_DEBUG", "SHN_EXT_BULK", "SHN_COUNT_SK_BITS", "SHN_HIP_LIB"} <= documented
