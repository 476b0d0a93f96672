"""Test-set cleaning from an embeddings cache: `python -m miclip.clean_testset`.

Counterpart of tools/cs_clean_testset.py (same subcommands, `score` flags,
defaults, CSV and summary dict), driving the GPU scorers of miclip.outliers:

    python -m miclip.clean_testset score CACHE_DIR OUT.csv [--method single|multi] ...

On top of the reference's flags, `score` takes --trim-frac / --trim-rounds
(single method: score against trimmed class centroids) and --kmeans
{sklearn,device} (multi method: where the k-means fit runs); given with the other
method they are a usage error, so nobody believes they trimmed. `select` and
`materialize` are declared and refused, as in the reference.
"""
import argparse
import sys
from pathlib import Path

# (flag, default, help): the integer `score` options, names and defaults of cs_clean_testset.py:47-82
_SCORE_INTS = (
    ("--k-fixed", 2, "multi: prototypes per class with --k-mode fixed"),
    ("--k-max", 4, "multi: cap on the prototypes per class in either k mode"),
    ("--min-samples-per-proto", 15, "multi: a class gets at most n / this many prototypes"),
    ("--random-state", 0, "multi: seed of the k-means fits"),
    ("--n-init", 10, "multi: k-means restarts per class"),
    ("--max-iter", 100, "multi: iteration limit of one k-means fit"),
)
_REFUSED = {
    "select": "`select` is not implemented yet. Use `score` for now.",
    "materialize": "`materialize` is not implemented yet. Use `score` for now.",
}


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog="python -m miclip.clean_testset",
                                     description="Score, select and materialize a cleaned test set from an embeddings cache")
    sub = parser.add_subparsers(dest="cmd", required=True)

    score = sub.add_parser("score", help="outlier scores of every cached row, written as CSV")
    score.add_argument("cache_dir", type=Path,
                       help="cache directory (embeddings.pt, labels.pt, metadata.csv)")
    score.add_argument("output", type=Path, help="where the score CSV goes")
    score.add_argument("--method", choices=["single", "multi"], default="single",
                       help="one centroid per class, or several k-means prototypes per class")
    score.add_argument("--k-mode", choices=["heuristic", "fixed"], default="heuristic",
                       help="multi: prototypes per class from the class size, or --k-fixed")
    for flag, default, text in _SCORE_INTS:
        score.add_argument(flag, type=int, default=default, help=text)
    score.add_argument("--trim-frac", type=float, default=None,
                       help="Single method: fraction of each class (0 <= f < 0.5) left out of "
                            "its centroid, lowest similarity first. Default: plain centroids.")
    score.add_argument("--trim-rounds", type=int, default=1,
                       help="Single method: trimming rounds (1..8) when --trim-frac is given.")
    score.add_argument("--kmeans", choices=["sklearn", "device"], default=None,
                       help="Multi method: k-means on the host (scikit-learn, the default) or on the GPU.")

    select = sub.add_parser("select", help="(not built) pick rows to remove from a score CSV")
    select.add_argument("scores_csv", type=Path, help="output of `score`")
    select.add_argument("rule_json", type=Path, help="selection rule as JSON")
    select.add_argument("output", type=Path, help="CSV of the rows picked")

    mat = sub.add_parser("materialize", help="(not built) lay out the cleaned test folder")
    mat.add_argument("source_images", type=Path, help="folder of the test images")
    mat.add_argument("index_csv", type=Path, help="index CSV that goes with the images")
    mat.add_argument("keep_list", type=Path,
                     help="CSV of the files to keep")
    mat.add_argument("output_dir", type=Path, help="folder to create")
    mat.add_argument("--invert", action="store_true",
                     help="keep_list names the files to leave out")
    mat.add_argument("--no-symlink", action="store_true",
                     help="copy the files, no symlinks")
    return parser


def run_score(args: argparse.Namespace):
    """The `score` subcommand: returns (scores frame, summary dict) after writing the CSV."""
    from . import outliers

    embeddings, labels, metadata = outliers.load_cache(outliers.resolve_cache_paths(args.cache_dir))
    if args.method == "single":
        scorer = outliers.SingleCentroidScorer(embeddings, labels, metadata)
        if args.trim_frac is None:
            centroids = scorer.compute_centroids()
        else:
            centroids = scorer.compute_centroids(trim_frac=args.trim_frac,
                                                 trim_rounds=args.trim_rounds)
        scores = scorer.score_centroid_distance(centroids=centroids)
        n_classes = len(centroids.centroids)
        summary = {"method": "single", "num_classes_present": int(n_classes),
                   "total_prototypes": int(n_classes)}
    else:
        scorer = outliers.MultiPrototypeScorer(embeddings, labels, metadata)
        prototypes = scorer.compute_prototypes(
            k_mode=args.k_mode, k_fixed=args.k_fixed, k_max=args.k_max,
            min_samples_per_proto=args.min_samples_per_proto, random_state=args.random_state,
            n_init=args.n_init, max_iter=args.max_iter, kmeans=args.kmeans)
        scores = scorer.score_prototype_distance(prototypes=prototypes)
        total = int(sum(prototypes.k_per_class.values()))
        n_classes = int(len(prototypes.prototypes))
        summary = {"method": "multi", "num_classes_present": n_classes,
                   "total_prototypes": total, "avg_k_per_class": float(total / max(1, n_classes))}
    output = Path(args.output)
    output.parent.mkdir(parents=True, exist_ok=True)
    scores.to_csv(output, index=False)
    summary = {"cache_dir": str(args.cache_dir), "output_csv": str(output),
               "num_samples": int(scores.shape[0]), **summary}
    print("\n==== Score Completed ====")
    print(summary)
    return scores, summary


def parse_args(argv=None) -> argparse.Namespace:
    """Parse, and refuse a flag that the chosen --method would ignore."""
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.cmd == "score":
        if args.method != "single" and (args.trim_frac is not None or args.trim_rounds != 1):
            parser.error("--trim-frac / --trim-rounds apply to --method single only")
        if args.method == "single" and args.trim_frac is None and args.trim_rounds != 1:
            parser.error("--trim-rounds needs --trim-frac")
        if args.method != "multi" and args.kmeans is not None:
            parser.error("--kmeans applies to --method multi only")
        if args.kmeans is None:
            args.kmeans = "sklearn"
    return args


def main(argv=None) -> int:
    args = parse_args(argv)
    if args.cmd in _REFUSED:
        raise NotImplementedError(_REFUSED[args.cmd])
    run_score(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
