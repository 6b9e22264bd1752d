"""Model files as texts: the eight-cable robot in the upstream YAML layout and a small generated SDF (tests/test_model_io.py,
tests/test_gpu_full_size.py)."""

EIGHT_YAML = """
cable: {radius: 0.005}
frame: {type: box, lower: [-0.3, -0.3, 0], upper: [0.3, 0.3, 0.6]}
joints:
  actuated: {damping: 1, effort: 100, min: 5, velocity: 10}
  passive: {damping: 0.01, effort: 100, velocity: 10}
platform:
  mass: 1
  inertia: [1, 1, 1, 0, 0, 0]
  position: {rpy: [0, 0, 0], xyz: [0, 0, 0.3]}
  size: [0.06, 0.06, 0.015]
points:
- {frame: [-0.3, -0.3, 0.6], platform: [0.03, -0.03, -0.0075]}
- {frame: [-0.3, 0.3, 0.6], platform: [-0.03, 0.03, -0.0075]}
- {frame: [0.3, 0.3, 0.6], platform: [0.03, 0.03, -0.0075]}
- {frame: [0.3, -0.3, 0.6], platform: [-0.03, -0.03, -0.0075]}
- {frame: [-0.3, -0.3, 0.0], platform: [-0.03, -0.03, 0.0075]}
- {frame: [-0.3, 0.3, 0.0], platform: [-0.03, 0.03, 0.0075]}
- {frame: [0.3, 0.3, 0.0], platform: [0.03, -0.03, 0.0075]}
- {frame: [0.3, -0.3, 0.0], platform: [0.03, 0.03, 0.0075]}
"""


def mini_sdf(anchors_f, anchors_p_world, plat_pose):
    links = "".join(
        f'<link name="virt_X{i}"><pose>{a[0]} {a[1]} {a[2]} 0 0 0</pose></link>'
        f'<link name="virt_Xpf{i}"><pose>{b[0]} {b[1]} {b[2]} 0 0 0</pose></link>'
        f'<joint name="cable{i}" type="prismatic"><parent>virt_Y{i}</parent><child>cable{i}</child><axis><xyz>0 0 1</xyz>'
        f"<limit><lower>-0.5</lower><upper>0.5</upper><effort>80</effort><velocity>10</velocity></limit>"
        f"<dynamics><damping>0.7</damping></dynamics></axis></joint>"
        for i, (a, b) in enumerate(zip(anchors_f, anchors_p_world))
    )
    return (
        '<?xml version="1.0"?><sdf version="1.4"><model name="m"><link name="frame"><pose>0 0 0 0 0 0</pose></link>'
        f'<link name="platform"><pose>{" ".join(str(v) for v in plat_pose)}</pose><inertial><inertia><ixx>1.5</ixx><iyy>2</iyy><izz>2.5</izz>'
        "<ixy>0.1</ixy><ixz>0</ixz><iyz>0</iyz></inertia><mass>3</mass></inertial></link>" + links + "</model></sdf>"
    )
