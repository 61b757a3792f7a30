"""Worker of test_gpu_patterns_bed_variants.py: extractPatternsBed over both fixtures in a fresh process, under the
EPIHIP_PAT_GROUP_BYTES value the parent put in the environment (the switches are read once per process)."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import helpers as H  # noqa: E402
import test_extract_patterns as TP  # noqa: E402
import test_gpu_patterns_bed as TB  # noqa: E402
import epialleler_amd as ea  # noqa: E402

BAM = os.path.join(H.GOLDEN, "bam")
groups = []
for bam, bed, total in (("capture.bam", "capture.bed", 2697), ("amplicon010meth.bam", "amplicon.bed", 942)):
    pb = ea.preprocessBam(os.path.join(BAM, bam))
    for kw in ({}, {"clip_patterns": True, "extract_context": "CX", "highlight_positions": [43125000, 61864584]}):
        reps = ea.extractPatternsBed(pb, os.path.join(BAM, bed), **kw)
        g = C.c_int64(0)
        ea._lib.check(ea._lib.load().epi_batch_extract_patterns_multi_stats(pb.batch(), C.byref(g), None, None))
        groups.append(g.value)
        n = 0
        for i, rep in enumerate(reps):
            tab = TP.table_from_report(rep)
            TB.same_table(tab, TP.oracle_patterns(bam=bam, bed=bed, bed_row=i + 1, **kw))
            n += len(tab["pattern"])
        assert kw or n == total, (bam, n)
print("groups", " ".join(str(g) for g in groups))
print("variant ok")
