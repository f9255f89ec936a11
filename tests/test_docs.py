"""-m "not gpu": the documents keep up with the code — every environment variable the library or the `plonkit` binary reads is
listed in INTEGRATION.md's table and every variable the table lists is read somewhere, every entry point include/plonkit_amd.h declares is in INTEGRATION.md's index."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def test_every_environment_variable_is_documented():
    csrc = os.path.join(ROOT, "plonkit_amd", "csrc")
    read = set()
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".cpp", ".h")):
            read |= set(re.findall(r'getenv\("((?:PLK|PLONKIT)_[A-Z0-9_]+)"\)', _read("plonkit_amd", "csrc", name)))
    assert len(read) >= 20, "the scan found suspiciously few variables: %s" % sorted(read)
    doc = _read("INTEGRATION.md")
    missing = sorted(v for v in read if "`%s`" % v not in doc)
    assert not missing, "read by the code, absent from INTEGRATION.md's table: %s" % missing
    # and the converse: a row whose variable nothing reads any more is stale
    table = doc[doc.index("## Environment variables"):]
    table = table[:table.index("\n## ", 1)]
    listed = set()
    for row in table.splitlines():
        if row.startswith("|"):
            listed |= set(re.findall(r"`(PLK_[A-Z0-9_]+)`", row.split("|")[1]))
    assert len(listed) >= 15, "the table scan found suspiciously few variables: %s" % sorted(listed)
    sources = [_read("bench.py")]
    for folder, _, names in os.walk(os.path.join(ROOT, "plonkit_amd")):
        sources += [_read(folder, n) for n in sorted(names) if n.endswith((".hip", ".cpp", ".h", ".py"))]
    stale = sorted(v for v in listed if not any('"%s"' % v in text for text in sources))
    assert not stale, "listed in INTEGRATION.md's table, read nowhere in plonkit_amd/ or bench.py: %s" % stale


def test_the_index_of_entry_points_is_current():
    """INTEGRATION.md's index (tools/abi_index.py) lists every function include/plonkit_amd.h declares, under the header section
    that names the reference interface it replaces"""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "abi_index.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    header = _read("include", "plonkit_amd.h")
    declared = set(re.findall(r"^\s*(?:const char \*|int32_t|uint64_t|uint32_t|void)\s*\**\s*(plk_[a-z0-9_]+)\s*\(", header, re.M))
    assert len(declared) >= 80
    doc = _read("INTEGRATION.md")
    index = doc[doc.index("abi-index:begin"): doc.index("abi-index:end")]
    missing = sorted(n for n in declared if "`%s`" % n not in index)
    assert not missing, missing
