"""Contour lines of dtm_whu.py's DTM (or of another raster of the grid) as ordered polylines: see ada_mvs_amd/contours.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.contours import main

if __name__ == "__main__":
    main()
