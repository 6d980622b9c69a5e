"""lidbox_amd: the lidbox pipeline on AMD Instinct GPUs (HIP kernels behind the reference's interfaces)."""


def iter_metadata_file(path, num_columns):
    """reference lidbox/__init__.py:41-46: the first `num_columns` space-separated columns of every line of a Kaldi-style
    metadata file (utt2path, id2label, ...); blank lines and lines starting with '#' are skipped.  The split is on single
    spaces, as in the reference: a value may hold spaces only where it is beyond the requested columns."""
    num_columns = int(num_columns)
    with open(path, encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            yield line.split(" ", num_columns)[:num_columns]
