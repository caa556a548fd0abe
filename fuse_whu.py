"""Depth-map fusion of a predict_whu.py output folder into one point cloud: see ada_mvs_amd/fusion.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.fusion import main

if __name__ == "__main__":
    main()
