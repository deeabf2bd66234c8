"""Drop-in alias: `import pycbinfer` resolves to the MI355X implementation in `cbinfer_amd`.

The reference's applications import `pycbinfer`, reach the classes as `pycbinfer.CBConv2d` and
`pycbinfer.conv2d.CBConv2d` (sceneLabeling/modelConverter.py:33, poseDetection/evalTools.py:91,101),
and its pickled models name `pycbinfer.conv2d.CBConv2d` / `CBPoolMax2d`; all of these resolve here.
"""
import sys

import cbinfer_amd
from cbinfer_amd import *            # noqa: F401,F403
from cbinfer_amd import CBChannelScale2d, CBSqueezeExcite, chanscale      # noqa: F401  (no entries of __all__)
from cbinfer_amd import CBGroupNorm2d, groupnorm      # noqa: F401  (likewise)
from cbinfer_amd import binary, chanreduce, conv2d, conv2d_cg, conv2d_fg, decoder, dwconv, groupconv, pad, pointwise, pool, rearrange, residual, resize, tconv

sys.modules[__name__ + '.conv2d'] = conv2d
sys.modules[__name__ + '.conv2d_cg'] = conv2d_cg
sys.modules[__name__ + '.conv2d_fg'] = conv2d_fg
sys.modules[__name__ + '.pool'] = pool
sys.modules[__name__ + '.residual'] = residual
sys.modules[__name__ + '.decoder'] = decoder
sys.modules[__name__ + '.tconv'] = tconv
sys.modules[__name__ + '.dwconv'] = dwconv
sys.modules[__name__ + '.pointwise'] = pointwise
sys.modules[__name__ + '.groupconv'] = groupconv
sys.modules[__name__ + '.rearrange'] = rearrange
sys.modules[__name__ + '.chanreduce'] = chanreduce
sys.modules[__name__ + '.resize'] = resize
sys.modules[__name__ + '.pad'] = pad
sys.modules[__name__ + '.binary'] = binary
sys.modules[__name__ + '.chanscale'] = chanscale
sys.modules[__name__ + '.groupnorm'] = groupnorm

__all__ = cbinfer_amd.__all__
