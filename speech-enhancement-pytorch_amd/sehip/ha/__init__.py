"""Hearing-aid back end (the reference's src/ha): NAL-R amplifier and compressor on the HIP path."""
from .amplifier import NALRTorch, fir_adjoint, fir_apply  # noqa: F401
from .compressor import CompressorTorch, compress_rows  # noqa: F401
from .stream import AmplifyStreamer  # noqa: F401
