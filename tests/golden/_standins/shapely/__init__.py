"""Stand-in for the two shapely primitives the reference's gap acceptance uses (see geometry.py).  Not shapely."""
