"""Pack the reference's data files that tests/test_datasets_cpu.py reads into tests/golden/reference_data/.

Run:  python tests/golden/make_reference_data.py <root of the reference checkout>

Each file is stored xz-compressed under its path relative to that root (`<path>.xz`); a compressed file above
the 1 MiB limit for a committed file is cut into `<path>.xz.00`, `<path>.xz.01`, ...  The test concatenates the
pieces and unpacks the tree into a temporary directory with the reference's own layout."""
import lzma
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_data")
PIECE = 1_000_000
FILES = ["data_pre_false/chameleon/raw/chameleon.npz",
         "data/squirrel/geom_gcn/raw/out1_graph_edges.txt",
         *[f"data/cora/raw/ind.cora.{s}" for s in ("x", "y", "tx", "ty", "allx", "ally", "graph", "test.index")],
         *[f"data/facebook100/{s}.mat" for s in ("Amherst41", "Reed98", "JohnsHopkins55")],
         *[f"data/twitch/DE/musae_DE_{s}" for s in ("edges.csv", "features.json", "target.csv")],
         *[f"data/{n}/{f}" for n in ("texas", "cornell", "wisconsin")
           for f in ("raw/out1_graph_edges.txt", "raw/out1_node_feature_label.txt", "processed/data.pt")],
         "mini/year0.pt"]


def main(ref):
    for rel in FILES:
        blob = lzma.compress(open(os.path.join(ref, rel), "rb").read(), preset=9 | lzma.PRESET_EXTREME)
        dst = os.path.join(OUT, rel + ".xz")
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        pieces = [blob[i:i + PIECE] for i in range(0, len(blob), PIECE)]
        names = [dst] if len(pieces) == 1 else [f"{dst}.{i:02d}" for i in range(len(pieces))]
        for name, piece in zip(names, pieces):
            with open(name, "wb") as f:
                f.write(piece)
        print(rel, len(blob), "bytes in", len(pieces), "piece(s)")


if __name__ == "__main__":
    main(sys.argv[1])
