"""CPU: the host side of the embedding-cache visualiser (miclip/embed_vis.py) -- the cache
loader's errors, the output file and its refusals, the pca_dim branches and the command
line -- with the device call stubbed out (there is no GPU here)."""
import numpy as np
import pandas as pd
import pytest
import torch

from miclip import embed_vis

N, D = 24, 12


def _write_cache(path, n=N, rows=None, labels=True, dtype=torch.float16):
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((n, D))).to(dtype)
    torch.save(x, path / "embeddings.pt")
    meta = pd.DataFrame({"file_name": [f"{i}.jpg" for i in range(rows or n)],
                         "ground_truth_word_label": ["a"] * (rows or n)})
    meta.to_csv(path / "metadata.csv", index=False)
    if labels:
        torch.save(torch.zeros(n, dtype=torch.long), path / "labels.pt")
    return x


@pytest.fixture
def stub(monkeypatch):
    """Replace the device t-SNE: records what it was given, returns ramp coordinates."""
    seen = []

    def fake(features, **kw):
        f = np.asarray(features.float() if isinstance(features, torch.Tensor) else features)
        seen.append((f, kw))
        coords = np.arange(2 * f.shape[0], dtype=np.float32).reshape(-1, 2)
        return embed_vis.TsneResult(coords, 0.5, 999, 50.0)
    monkeypatch.setattr(embed_vis, "tsne", fake)
    return seen


def test_load_cache_errors_and_optional_labels(tmp_path):
    with pytest.raises(FileNotFoundError, match="Missing embeddings file: .*embeddings.pt"):
        embed_vis.load_cache(tmp_path)
    torch.save(torch.zeros(3, 4), tmp_path / "embeddings.pt")
    with pytest.raises(FileNotFoundError, match="Missing metadata file: .*metadata.csv"):
        embed_vis.load_cache(tmp_path)
    _write_cache(tmp_path, labels=False)
    emb, meta, lab = embed_vis.load_cache(str(tmp_path))
    assert emb.shape == (N, D) and emb.dtype == torch.float16 and len(meta) == N and lab is None
    _write_cache(tmp_path)
    assert embed_vis.load_cache(tmp_path)[2].shape == (N,)


def test_output_file_overwrite_and_columns(tmp_path, stub):
    x = _write_cache(tmp_path)
    df = embed_vis.visualize_cache(tmp_path, out_prefix="run1", seed=7, device="cpu",
                                   perplexity=5.0)
    coords = np.load(tmp_path / "run1_tsne_coords.npy")
    assert coords.shape == (N, 2) and coords.dtype == np.float32
    assert list(df.columns) == ["file_name", "ground_truth_word_label", "x", "y"]
    assert np.array_equal(df["x"].to_numpy(), coords[:, 0])
    assert np.array_equal(df["y"].to_numpy(), coords[:, 1])
    feats, kw = stub[0]
    assert np.array_equal(feats, x.float().numpy())          # no PCA: the cache as it is
    assert kw == {"seed": 7, "device": "cpu", "perplexity": 5.0}
    with pytest.raises(FileExistsError, match=r"Output exists: .*run1_tsne_coords.npy "
                                              r"\(use --overwrite to replace\)"):
        embed_vis.visualize_cache(tmp_path, out_prefix="run1", device="cpu")
    assert len(stub) == 1                                    # refused before any device work
    embed_vis.visualize_cache(tmp_path, out_prefix="run1", overwrite=True, device="cpu")
    assert len(stub) == 2


def test_row_mismatch_raises_the_references_error(tmp_path, stub):
    _write_cache(tmp_path, rows=N - 1)
    with pytest.raises(ValueError, match=f"Row mismatch: coords_2d has {N} rows, "
                                         f"metadata has {N - 1} rows."):
        embed_vis.visualize_cache(tmp_path, device="cpu")
    assert (tmp_path / "vis_tsne_coords.npy").is_file()      # saved first, as the reference does


def test_pca_dim_branches(tmp_path, stub, capsys):
    x = _write_cache(tmp_path)
    with pytest.raises(ValueError, match="pca_dim must be a positive integer."):
        embed_vis.visualize_cache(tmp_path, pca_dim=0, device="cpu")
    embed_vis.visualize_cache(tmp_path, pca_dim=D, out_prefix="skip", device="cpu")
    assert f"[warn] pca_dim={D} >= embedding_dim={D}; skipping PCA." in capsys.readouterr().out
    assert np.array_equal(stub[-1][0], x.float().numpy())
    embed_vis.visualize_cache(tmp_path, pca_dim=4, out_prefix="pca4", device="cpu")
    assert "pca_explained_variance_ratio_sum" in capsys.readouterr().out
    assert stub[-1][0].shape == (N, 4) and stub[-1][0].dtype == np.float32


def test_pca_reduce_matches_sklearn_on_the_host():
    from sklearn.decomposition import PCA
    x = np.random.default_rng(1).standard_normal((40, 10)) * np.linspace(3, 0.3, 10)
    got, ratio = embed_vis.pca_reduce(x.astype(np.float32), 3, device="cpu")
    pca = PCA(n_components=3, svd_solver="full")
    want = pca.fit_transform(x.astype(np.float32).astype(np.float64))
    assert got.dtype == np.float32 and got.shape == (40, 3)
    for k in range(3):
        assert min(np.abs(got[:, k] - want[:, k]).max(),
                   np.abs(got[:, k] + want[:, k]).max()) <= 1e-4
    assert abs(ratio - pca.explained_variance_ratio_.sum()) <= 1e-5
    for bad in (0, -3):
        with pytest.raises(ValueError, match="pca_dim must be a positive integer."):
            embed_vis.pca_reduce(x, bad, device="cpu")


def test_umap_is_refused_and_flags_are_the_references(tmp_path, stub, capsys):
    _write_cache(tmp_path)
    with pytest.raises(NotImplementedError, match="umap-learn is not available"):
        embed_vis.main(["--cache_dir", str(tmp_path), "--umap"])
    with pytest.raises(SystemExit):                           # one of --umap / --tsne is required
        embed_vis.main(["--cache_dir", str(tmp_path)])
    embed_vis.main(["--cache_dir", str(tmp_path), "--tsne", "--tsne_perplexity", "7",
                    "--tsne_metric", "euclidean", "--tsne_init", "random", "--seed", "3",
                    "--out_prefix", "cli", "--color_by", "file_name", "--hover", "file_name",
                    "--umap_neighbors", "5", "--umap_min_dist", "0.2", "--umap_metric", "cosine"])
    assert "accepted and ignored" in capsys.readouterr().out
    assert (tmp_path / "cli_tsne_coords.npy").is_file()
    assert stub[-1][1] == {"seed": 3, "device": None, "perplexity": 7.0, "metric": "euclidean",
                           "init": "random"}


def test_random_init_is_bit_equal_to_sklearns():
    """TSNE._fit: 1e-4 * random_state.standard_normal(size=(n, 2)).astype(float32), compared
    bit for bit."""
    from sklearn.utils import check_random_state
    for seed, n in ((1, 33), (42, 257)):
        want = 1e-4 * check_random_state(seed).standard_normal(size=(n, 2)).astype(np.float32)
        got = embed_vis.random_init(n, seed)
        assert got.dtype == np.float32 and np.array_equal(got, want)


def test_host_validation_comes_before_any_launch():
    x = np.random.default_rng(0).standard_normal((20, 8)).astype(np.float32)
    bad = x.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        embed_vis.tsne(bad, perplexity=5.0, device="cpu")
    with pytest.raises(ValueError, match="perplexity"):
        embed_vis.tsne(x, perplexity=20.0, device="cpu")
    with pytest.raises(ValueError, match="metric"):
        embed_vis.tsne(x, perplexity=5.0, metric="manhattan", device="cpu")
    with pytest.raises(ValueError, match="N must be in"):
        embed_vis.tsne(x[:3], perplexity=2.0, device="cpu")
    with pytest.raises(ValueError, match='init="pca" cannot be used with metric="precomputed"'):
        embed_vis.tsne(np.abs(x[:, :8] @ x[:, :8].T)[:8, :8], perplexity=2.0,
                       metric="precomputed", device="cpu")
    with pytest.raises(ValueError, match="init must have shape"):
        embed_vis.tsne(x, perplexity=5.0, init=np.zeros((5, 2)), device="cpu")
