"""Filter the fused cloud on the GPU (k-NN outlier removal, normals): see ada_mvs_amd/cloud_filter.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.cloud_filter import main

if __name__ == "__main__":
    main()
