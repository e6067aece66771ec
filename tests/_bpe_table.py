"""A CLIP BPE merge table rebuilt from tests/golden/bpe_merges_subset.npz, for the tokenizer tests.

The published table (bpe_simple_vocab_16e6.txt.gz, 1.3 MB) is third-party data the repository does not carry.  The fixture keeps the merges the
tokenizer consults on the test strings (tests/golden/gen_golden.py `bpe_merges_subset`), each with its rank.  Token ids are rank + 512, so a table
that holds each kept merge at its rank, and at every other rank a pair that no byte sequence forms, gives the published ids for those strings."""
import gzip
import os

import numpy as np

N_MERGES = 49152 - 256 - 2                        # merges the tokenizer reads: 49 408 ids = 512 byte symbols + 48 894 merges + 2 special tokens
FILLER = "\u2400{} \u2401"            # symbols outside the byte alphabet: never formed, joined strings unique per rank
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bpe_merges_subset.npz")


def write_table(path, ranks, merges):
    lines = [FILLER.format(r) for r in range(N_MERGES)]
    for r, m in zip(ranks, merges):
        lines[int(r)] = str(m)
    with gzip.open(path, "wt", encoding="utf-8") as f:
        f.write("\n".join(["#version: 0.2"] + lines) + "\n")
    return path


def write_fixture_table(path):
    g = np.load(FIXTURE)
    return write_table(path, g["ranks"], g["merges"])
