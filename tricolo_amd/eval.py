"""Score a saved prediction file: the reference's eval.py (`python eval.py data=... +prediction_file_path=output.p`).

    python -m tricolo_amd.eval data=text2shape_chair_table +prediction_file_path=output.p [+nearest_path=nearest.jsonl] [+direction=both]

Unpickles the embeddings dict that tricolo_amd.test (or the reference's test.py) wrote and prints compute_metrics' `RR@1 RR@5 NDCG@5
MRR` line; with +nearest_path= the nearest.jsonl of evaluation.shape_f1 is written too.  +direction=s2t|both (or +inference.direction=)
scores the shape -> text direction as well: a second `S2T RR@1 RR@5 NDCG@5 MRR` line, records in nearest_s2t.jsonl beside nearest_path,
the numbers under "s2t" of the returned dict (evaluation.eval_retrieval.compute_metrics).  The reference also passes
`metric=cfg.evaluation.metric`, an argument its own compute_metrics does not have: it is not read here.  main() returns the metrics dict.
"""
import pickle
import sys

from . import config as tcfg
from .evaluation.eval_retrieval import compute_metrics


def parse(argv=None):
    """-> (cfg, prediction_file_path, nearest_path | None)"""
    cfg = tcfg.compose(overrides=list(argv if argv is not None else sys.argv[1:]))
    path = cfg.get("prediction_file_path")
    if not path:
        raise SystemExit("tricolo_amd.eval: +prediction_file_path=FILE (the output.p of tricolo_amd.test) is required")
    return cfg, str(path), (str(cfg.nearest_path) if cfg.get("nearest_path") else None)


def main(argv=None):
    cfg, path, nearest_path = parse(argv)
    with open(path, "rb") as f:
        embeddings_dict = pickle.load(f)
    direction = str(cfg.get("direction") or cfg.inference.get("direction", "t2s"))
    return compute_metrics(cfg.data.dataset, embeddings_dict, print_results=True, nearest_path=nearest_path, direction=direction)


if __name__ == "__main__":
    main()
