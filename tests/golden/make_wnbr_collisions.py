"""Regenerates wnbr_collisions.json: per k of wnbr_ref.KS, the pairs of different canonical interiors (k - 2 bases) whose index hashes (the numpy
port in tests/wnbr_ref.py) agree in the tag (high 32 bits) and in the home slot of a 1024-slot index (low 10 bits); `seam_pairs`: the same among interiors that share their last 31 bases (k = 47, 62, 63).  A birthday search over 2^23
random interiors per k, fixed seeds, a few seconds per k; tests/test_wnbr_ref_cpu.py asserts the property of every pair it reads.

    python tests/golden/make_wnbr_collisions.py"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import wnbr_ref as W  # noqa: E402

SEED, DRAWS = 20240, 1 << 23


def main():
    pairs, secs = {}, {}
    for k in W.KS:
        t0 = time.time()
        found = W.collision_search(k, SEED + k, DRAWS)
        secs[k] = time.time() - t0
        assert found, "no pair at k = %d: try another seed" % k
        pairs[str(k)] = [["%x" % a, "%x" % b] for a, b in found[:4]]
        print("k = %d: %d pairs in %.1f s" % (k, len(found), secs[k]))
    seam = {}
    for k in W.SEAM_KS:                                     # the same among interiors that share their last 31 bases
        t0 = time.time()
        found = []
        for j in range(8):                                  # (only the draws that are canonical as drawn count, about half: a quarter of the pairs)
            found = W.collision_search(k, SEED + 100 + k + 1000 * j, DRAWS, same_low=True)
            if found:
                break
        assert found, "no seam pair at k = %d: try another seed" % k
        seam[str(k)] = [["%x" % a, "%x" % b] for a, b in found[:4]]
        print("k = %d, same last 31 bases: %d pairs in %.1f s" % (k, len(found), time.time() - t0))
    with open(W.COLLISIONS, "w") as f:
        json.dump(dict(seed=SEED, draws=DRAWS, slot_bits=10, tag_bits=32, pairs=pairs, seam_pairs=seam), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
