"""Align a cloud or mesh to a truth by point-to-plane ICP on the GPU, before accuracy_whu.py scores it: see ada_mvs_amd/register.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.register import main

if __name__ == "__main__":
    main()
