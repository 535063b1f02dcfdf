#!/usr/bin/env python3
"""Extract the multisearch result fixture (DATA only) from a checkout of the reference.

    python tests/golden/make_multisearch_golden.py PATH/TO/kmerseek

Reads tests/testdata/index/ced9-bcl2-first25.hp.k16.manysearch.csv — the 16-column result file the reference keeps, with the
columns its do_multisearch (src/python/kmerseek/search.py:144-158) adds: prob_overlap, prob_overlap_adjusted,
containment_adjusted, containment_adjusted_log10, tf_idf_score — and writes tests/golden/multisearch_expected.json: the column
names in the file's order and its rows, every value as the string the file holds.  Nothing of the reference is executed."""
import csv
import json
import os
import sys

OUT = os.path.dirname(os.path.abspath(__file__))
REL = os.path.join("tests", "testdata", "index", "ced9-bcl2-first25.hp.k16.manysearch.csv")


def main(ref):
    with open(os.path.join(ref, REL), newline="") as f:
        rows = list(csv.reader(f))
    columns, rows = rows[0], rows[1:]
    assert len(columns) == 16 and len(rows) == 5 and all(len(r) == 16 for r in rows)
    out = {"source": REL.replace(os.sep, "/"), "query_fasta": "ced9.fasta",
           "target_fasta": "bcl2_first25_uniprotkb_accession_O43236_OR_accession_2025_02_06.fasta.gz",
           "moltype": "hp", "ksize": 16, "scaled": 5, "columns": columns, "rows": [dict(zip(columns, r)) for r in rows]}
    path = os.path.join(OUT, "multisearch_expected.json")
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
