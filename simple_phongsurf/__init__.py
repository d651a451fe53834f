"""Import-name alias for the reference's `simple_phongsurf` package (model/baseline/splattingavatar.py: `PhongSurfacePy3d`)."""
from fateavatar_amd.phongsurf import PhongSurface as PhongSurfacePy3d  # noqa: F401

__all__ = ["PhongSurfacePy3d"]
