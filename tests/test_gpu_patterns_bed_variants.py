"""EPIHIP_PAT_GROUP_BYTES (the scratch cap of a group of targets in epi_batch_extract_patterns_multi) is result-neutral:
the fixtures' tables equal the oracle's in a fresh process under every value, and the cap does cut the targets into the
groups it should."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("cap,least,most", [
    (None, 1, 1),                 # the default (256 MiB): one group
    ("0", 1, 1),                  # 0 and negative values: the default
    ("-5", 1, 1),
    ("1000000", 2, 565),          # ~1 MB: a few groups
    ("20000", 10, 565),           # 20 kB: a few targets per group
    ("1", 565, 565),              # below every single target: each runs alone
])
def test_group_cap_variants(cap, least, most):
    e = dict(os.environ)
    e.pop("EPIHIP_PAT_GROUP_BYTES", None)
    if cap is not None:
        e["EPIHIP_PAT_GROUP_BYTES"] = cap
    r = subprocess.run([sys.executable, os.path.join(HERE, "_patterns_bed_worker.py")], env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "variant ok" in r.stdout
    groups = [int(g) for g in [ln for ln in r.stdout.splitlines() if ln.startswith("groups ")][0].split()[1:]]
    assert least <= groups[0] <= most and least <= groups[1] <= most      # capture.bed
    assert all(1 <= g <= 4 for g in groups[2:])                            # amplicon.bed
