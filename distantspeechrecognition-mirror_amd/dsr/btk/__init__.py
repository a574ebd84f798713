"""Python face of the BTK operators with the reference's SWIG-visible names (btk/*/*.i): every class X is exposed
as XPtr(...), `for v in stream` calls reset() then next() until the end-of-stream error becomes StopIteration
(btk/stream/stream.i:111-115, btk/include/jexception.i:178-180).
Modules: stream, feature, modulated, beamformer, postfilter, dereverberation, cancelVP, convolution, sad; mkBeamforming (btk/lib/mkBeamforming.py:
the maximum empirical kurtosis beamformers, imported on demand); mnBeamforming and GGDcEst (btk/lib/mnBeamforming.py, btk/lib/GGDcEst.py: the maximum
negentropy beamformers and the generalised Gaussian model they need, imported on demand)."""
from . import cancelVP  # noqa: F401  the echo cancellers (btk/cancelVP/cancelVP.i)
from . import convolution  # noqa: F401  OverlapAdd / OverlapSave (btk/convolution/convolution.i)
from . import sad  # noqa: F401  speech activity detection (btk/sad/sad.i)
