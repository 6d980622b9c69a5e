"""Counterpart of lidbox/embed: the scikit-learn style back-end for embedding vectors, on the HIP device."""
from . import sklearn_utils  # noqa: F401
