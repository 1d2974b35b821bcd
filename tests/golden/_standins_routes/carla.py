"""Stand-in for what the reference's path planner uses of CARLA once the graph is given: ``Location`` with ``distance`` (the
Euclidean distance in 3-D, float64) and the ``LaneType`` names.  Kept in a directory of its own: tests/golden/_standins/carla.py
serves the ring generator and stays as it is.  Not CARLA."""
import math


class Location:
    def __init__(self, x=0.0, y=0.0, z=0.0):
        self.x, self.y, self.z = float(x), float(y), float(z)

    def distance(self, other):
        return math.sqrt((self.x - other.x) ** 2 + (self.y - other.y) ** 2 + (self.z - other.z) ** 2)


class LaneType:
    Driving = "Driving"
    Sidewalk = "Sidewalk"
    Shoulder = "Shoulder"
