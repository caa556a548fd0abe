"""Tree tops and crown outlines from dtm_whu.py's nDSM and buildings_whu.py's labels: see ada_mvs_amd/trees.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.trees import main

if __name__ == "__main__":
    main()
