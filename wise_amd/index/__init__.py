"""The vector indexes.  `from wise_amd.index import IVFSQIPIndex` resolves on first use, so importing a light submodule
(faiss_io) does not pull in torch."""

__all__ = ["IVFSQIPIndex"]


def __getattr__(name):
    if name == "IVFSQIPIndex":
        from .ivf_sq import IVFSQIPIndex
        return IVFSQIPIndex
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
