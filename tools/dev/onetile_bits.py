"""Records tests/golden/onetile_update_bits.json: SHA-256 of the table and the losses of every case of
tests/onetile_cases.py, computed with the library GE_LIB names (the parent commit's, built next to the product one with
tools/dev/build_variant.py or from a worktree); the product library when GE_LIB is not set.  Every case runs twice and a
case that does not reproduce itself is recorded as null.
usage (GPU box): GE_LIB=graphembeddings_amd/_variants/libge_parent.so python tools/dev/onetile_bits.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if os.environ.get("GE_LIB"):
    from graphembeddings_amd import _lib as _L
    _L.LIB_PATH = os.path.abspath(os.environ["GE_LIB"])
import onetile_cases as C

out = {}
for model in C.MODELS:
    for margin in C.MARGINS:
        (a, live), (b, _) = C.run_det(model, margin), C.run_det(model, margin)
        out[C.det_key(model, margin)] = a if a == b else None
        print("det", model, margin, "reproduced" if a == b else "NOT reproduced", "live", live, flush=True)
    for margin in C.PLAIN_MARGINS:
        (a, _, live), (b, _, _) = C.run_plain(model, margin), C.run_plain(model, margin)
        out[C.plain_key(model, margin)] = a if a == b else None
        print("plain", model, margin, "reproduced" if a == b else "NOT reproduced", "live", live, flush=True)
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "onetile_update_bits.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(out, sort_keys=True))
