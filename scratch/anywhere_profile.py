"""Wall time of preprocessBam(F, mates="anywhere") against preprocessBam(G(F)), interleaved, plus equality."""
import json
import sys
import time

import numpy as np

import epialleler_amd as ea

F, G, reps = sys.argv[1], sys.argv[2], int(sys.argv[3])
a = ea.preprocessBam(F, mates="anywhere", nthreads=16)
b = ea.preprocessBam(G, nthreads=16)
for k in ("xm", "off", "rname", "strand", "start"):
    assert np.array_equal(a.host[k], b.host[k]), k
assert (a.n, a.nrecs) == (b.n, b.nrecs)
res = {"templates": a.n, "records": a.nrecs, "bytes": a.nbytes, "anywhere_s": [], "adjacent_twin_s": []}
del a, b
for _ in range(reps):
    t = time.perf_counter(); x = ea.preprocessBam(F, mates="anywhere", nthreads=16); res["anywhere_s"].append(time.perf_counter() - t); del x
    t = time.perf_counter(); x = ea.preprocessBam(G, nthreads=16); res["adjacent_twin_s"].append(time.perf_counter() - t); del x
res["anywhere_median_s"] = float(np.median(res["anywhere_s"]))
res["adjacent_twin_median_s"] = float(np.median(res["adjacent_twin_s"]))
print(json.dumps(res))
