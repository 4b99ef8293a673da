#!/usr/bin/env python3
"""Generate tests/golden/training_chunk.npz -- one training chunk of the data writer, as the REFERENCE's reader parses it.

Dev container only: needs the reference's training reader (train/torch/data.py of a reference source tree).  One
self-play game with one worker is a pure function of its seed (tests/test_search_cpu.py::test_golden_dummy_backend_games),
so its tdata chunk is too.  Stored: the chunk text
(zlib) and, per record, the fields the reference's Data.parse() produced from it.
tests/test_search_cpu.py::test_training_chunks_parse_with_reference_reader plays the same game and requires the
writer to emit the same text byte for byte.

    python tests/golden/make_golden_chunks.py <reference source tree>
"""
from __future__ import annotations

import glob
import gzip
import io
import os
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden_specs import TRAINING_CHUNK_GAME  # noqa: E402
from sayuri_amd import search as S  # noqa: E402

FIELDS = ("version", "mode", "board_size", "komi", "rule", "wave", "to_move", "result", "final_score",
          "avg_q", "avg_score", "q_stddev", "score_stddev")


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.join(sys.argv[1], "train", "torch"))
    import data as refdata
    with tempfile.TemporaryDirectory() as d:
        S.selfplay(None, dict(TRAINING_CHUNK_GAME, target_directory=d))
        raw = gzip.open(sorted(glob.glob(os.path.join(d, "tdata", "*", "*.gz")))[0]).read()
    stream, recs = io.StringIO(raw.decode()), []
    while True:
        r = refdata.Data()
        if not r.load_from_stream(stream):
            break
        r.parse()
        recs.append(r)
    out = {"text": np.frombuffer(zlib.compress(raw, 9), np.uint8)}
    for f in FIELDS:
        out[f] = np.array([getattr(r, f) for r in recs], np.float64)
    out["planes"] = np.stack([np.asarray(r.planes) for r in recs]).astype(np.uint8)
    for f in ("prob", "aux_prob", "ownership"):
        out[f] = np.stack([np.asarray(getattr(r, f)) for r in recs]).astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "training_chunk.npz"), **out)
    print(f"training_chunk.npz: {len(recs)} records, {len(raw)} bytes of text")


if __name__ == "__main__":
    main()
