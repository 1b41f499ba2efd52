"""The scratch blocks of a matcher handle (OrbmSlot) and of a vocabulary handle (OrbvSlot) are picked by NAME: no host file
indexes d_buf / d_cap with a number, reserves a numbered block or gives a slot enumerator a value (DESIGN.md "Scratch
blocks have names")."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orbslamm_amd", "csrc")


def host_sources():
    files = sorted(set(glob.glob(os.path.join(CSRC, "*_host.inc")) + glob.glob(os.path.join(CSRC, "*.inc"))))
    assert len(files) >= 10
    # comments may speak of numbers; code may not
    return {os.path.basename(f): re.sub(r"//[^\n]*|/\*.*?\*/", "", open(f).read(), flags=re.S) for f in files}


def hits(pattern):
    return [(name, m.group(0)) for name, src in host_sources().items() for m in re.finditer(pattern, src)]


def test_no_block_is_indexed_by_a_literal():
    assert hits(r"\bd_(?:buf|cap)\s*\[\s*\d[^\]]*\]") == []


def test_no_reserve_takes_a_literal_slot():
    assert hits(r"\borb[mv]_reserve\s*\(\s*[^,()]+,\s*\d[^,)]*") == []


def test_no_slot_enumerator_carries_a_number():
    assert hits(r"\b(?:S|G|T|SV)_[A-Z0-9_]+\s*=\s*\d+") == []


def test_tables_are_sized_by_the_enum_counts():
    src = host_sources()
    for name, count in (("orbm_host.inc", "ORBM_SLOT_COUNT"), ("orbv_host.inc", "SV_COUNT")):
        sizes = re.findall(r"\bd_(?:buf|cap)\s*\[([^\]]*)\]\s*=", src[name])
        assert sizes == [count, count], (name, sizes)
        enum = re.search(r"enum\s+\w+\s*\{([^}]*)\}", src[name]).group(1)
        assert [e.strip() for e in enum.split(",") if e.strip()][-1] == count
    # and no other file declares such a table
    assert all(not re.search(r"\bd_(?:buf|cap)\s*\[[^\]]*\]\s*=", s) for n, s in src.items() if n not in ("orbm_host.inc", "orbv_host.inc"))
