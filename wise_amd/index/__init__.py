"""The vector indexes.  `from wise_amd.index import IVFSQIPIndex` resolves on first use, so importing a light submodule
(faiss_io) does not pull in torch."""

__all__ = ["IVFSQIPIndex", "IVFSQfp16IPIndex"]


def __getattr__(name):
    if name in __all__:
        from . import ivf_sq
        return getattr(ivf_sq, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
