"""Stand-in for the three CARLA classes the reference's ring generator uses: ``Location``, ``Rotation`` and ``Transform`` with
``transform()`` as CARLA's Python API documents it -- the point is rotated by the transform's rotation (degrees; yaw about z,
then pitch about y, then roll about x, in the simulator's left-handed frame) and then translated by its location.  float64
throughout (the simulator itself holds float32).  Not CARLA."""
import math


class Location:
    def __init__(self, x=0.0, y=0.0, z=0.0):
        self.x, self.y, self.z = float(x), float(y), float(z)


class Rotation:
    def __init__(self, pitch=0.0, yaw=0.0, roll=0.0):
        self.pitch, self.yaw, self.roll = float(pitch), float(yaw), float(roll)


class Transform:
    def __init__(self, location=None, rotation=None):
        self.location = location if location is not None else Location()
        self.rotation = rotation if rotation is not None else Rotation()

    def transform(self, in_point):
        cy, sy = math.cos(math.radians(self.rotation.yaw)), math.sin(math.radians(self.rotation.yaw))
        cr, sr = math.cos(math.radians(self.rotation.roll)), math.sin(math.radians(self.rotation.roll))
        cp, sp = math.cos(math.radians(self.rotation.pitch)), math.sin(math.radians(self.rotation.pitch))
        x, y, z = in_point.x, in_point.y, in_point.z
        out = Location(x * (cp * cy) + y * (cy * sp * sr - sy * cr) + z * (-cy * sp * cr - sy * sr),
                       x * (cp * sy) + y * (sy * sp * sr + cy * cr) + z * (-sy * sp * cr + cy * sr),
                       x * sp + y * (-cp * sr) + z * (cp * cr))
        out.x += self.location.x
        out.y += self.location.y
        out.z += self.location.z
        return out
