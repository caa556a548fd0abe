"""Building footprints from dtm_whu.py's nDSM as polygons with heights: see ada_mvs_amd/buildings.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.buildings import main

if __name__ == "__main__":
    main()
