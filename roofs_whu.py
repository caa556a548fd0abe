"""Roof planes of the buildings of buildings_whu.py, as polygons with pitch, aspect and area: see ada_mvs_amd/roofs.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.roofs import main

if __name__ == "__main__":
    main()
