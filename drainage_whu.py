"""The drainage network of dtm_whu.py's DTM (or of another raster of the grid): fill, D8 directions, accumulation, basins, streams:
see ada_mvs_amd/drainage.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.drainage import main

if __name__ == "__main__":
    main()
