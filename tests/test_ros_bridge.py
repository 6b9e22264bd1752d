"""the rospy bridge around the facade, against a FAKE rospy (ROS is not in the image): topic names,
message types and field mapping of CdprGazeboPlugin.cpp:176-198, 248-280, wrong-length Joys dropped, per-robot
namespaces for a batch.  The facade is replaced by a stub that only has what the bridge touches (bus, config, engine
clock), so this runs without a GPU; the end-to-end run with the real engine is in tests/test_gpu_parity.py."""
import sys
import types

import numpy as np
import pytest

from fake_ros import install_fake_ros


class StubFacade:
    """What the bridge needs of CdprGazeboPlugin: the bus, the config, update() and the engine's clock."""

    def __init__(self, pkg, B, per_robot=False):
        self.bus = pkg.TopicBus()
        self.config = pkg.Config(batch=B, perRobotCommands=per_robot)
        self.engine = types.SimpleNamespace(sim_time=0.0)
        self.joys = []
        self.bus.subscribe("jointVelocities", lambda m: self.joys.append(("v", m)))
        self.bus.subscribe("jointPositions", lambda m: self.joys.append(("p", m)))
        self.updates = 0

    def update(self, n=1):
        self.updates += n
        self.engine.sim_time += n * self.config.dt


def test_single_robot_topics_and_field_mapping(pkg, monkeypatch):
    from cdpr_simulation_amd.ros_bridge import CdprRosBridge

    log = install_fake_ros(monkeypatch)
    f = StubFacade(pkg, 1)
    br = CdprRosBridge(f, publish_clock=True)
    assert log["node"] == "cdpr_gazebo_simulator"
    assert sorted(br.topics()) == sorted(["jointVelocities", "jointPositions", "jointStates", "platformPose", "wireStates", "pid"])
    assert log["pubs"]["jointStates"].queue_size == 256 and log["subs"]["jointVelocities"].queue_size == 256  # PLG.h:21-22
    # ROS -> facade: a 4-axis Joy goes through, a 3-axis one is dropped (PLG.cpp:68-73)
    Joy = sys.modules["sensor_msgs.msg"].Joy
    log["subs"]["jointVelocities"].deliver(Joy(axes=[0.01, 0.02, 0.03, 0.04]))
    log["subs"]["jointPositions"].deliver(Joy(axes=[0.1, 0.2, 0.3]))
    br.step(3)
    assert f.updates == 3 and len(f.joys) == 1 and f.joys[0][0] == "v"
    assert np.allclose(f.joys[0][1].axes, [[0.01, 0.02, 0.03, 0.04]]) and f.joys[0][1].robots is None
    assert abs(log["pubs"]["/clock"].sent[-1].clock.to_sec() - 0.003) < 1e-12
    # facade -> ROS
    names = ["cable0", "cable1", "cable2", "cable3"]
    f.bus.publish("jointStates", pkg.JointState(name=names, position=np.arange(4.0)[None], velocity=-np.arange(4.0)[None],
                                               effort=10 * np.arange(4.0)[None], header=pkg.Header(stamp=0.25)))
    js = log["pubs"]["jointStates"].sent[-1]
    assert js.name == names and js.position == [0.0, 1.0, 2.0, 3.0] and js.velocity[3] == -3.0 and js.effort[2] == 20.0
    assert js.header.stamp.to_sec() == 0.25
    f.bus.publish("platformPose", pkg.PlatformState(pose=pkg.Pose(position=np.array([[1.0, 2.0, 3.0]]), orientation=np.array([[0.1, 0.2, 0.3, 0.9]])),
                                                    velocity=pkg.Twist(linear=np.array([[4.0, 5.0, 6.0]]), angular=np.array([[7.0, 8.0, 9.0]])),
                                                    header=pkg.Header(stamp=0.5)))
    ps = log["pubs"]["platformPose"].sent[-1]
    assert (ps.pose.position.x, ps.pose.position.y, ps.pose.position.z) == (1.0, 2.0, 3.0)
    assert (ps.pose.orientation.x, ps.pose.orientation.y, ps.pose.orientation.z, ps.pose.orientation.w) == (0.1, 0.2, 0.3, 0.9)  # PLG.cpp:266-269
    assert (ps.velocity.linear.x, ps.velocity.angular.z) == (4.0, 9.0)
    f.bus.publish("wireStates", pkg.WireStates(stateChange=pkg.KeyValue(key="cable2", value="slack"), header=pkg.Header(stamp=0.75)))
    ws = log["pubs"]["wireStates"].sent[-1]
    assert (ws.stateChange.key, ws.stateChange.value, ws.header.stamp.to_sec()) == ("cable2", "slack", 0.75)
    f.bus.publish("pid", pkg.Joy(axes=np.arange(9.0)[None], header=pkg.Header(stamp=1.0)))
    assert log["pubs"]["pid"].sent[-1].axes == [float(i) for i in range(9)]


def test_batch_uses_one_namespace_per_robot_and_masks_partial_arrivals(pkg, monkeypatch):
    from cdpr_simulation_amd.ros_bridge import CdprRosBridge

    log = install_fake_ros(monkeypatch)
    f = StubFacade(pkg, 3, per_robot=True)
    br = CdprRosBridge(f, namespace="/sim", init_node=False)
    assert "/sim/robot2/jointStates" in br.topics() and log["node"] is None
    Joy = sys.modules["sensor_msgs.msg"].Joy
    log["subs"]["/sim/robot1/jointVelocities"].deliver(Joy(axes=[0.1, 0.1, 0.1, 0.1]))
    br.step()
    kind, joy = f.joys[-1]
    assert kind == "v" and list(joy.robots) == [0, 1, 0] and np.allclose(joy.axes[1], 0.1) and np.allclose(joy.axes[0], 0.0)
    for b in range(3):
        log["subs"][f"/sim/robot{b}/jointPositions"].deliver(Joy(axes=[0.01 * b] * 4))
    br.step()
    kind, joy = f.joys[-1]
    assert kind == "p" and joy.robots is None and np.allclose(joy.axes[:, 0], [0.0, 0.01, 0.02])  # every robot heard: a plain batch
    eff = np.array([[1.0, 2.0, 3.0, 4.0]] * 3)
    f.bus.publish("jointStates", pkg.JointState(name=["cable0"] * 4, position=eff, velocity=eff, effort=eff * [[1], [2], [3]], header=pkg.Header(stamp=0.1)))
    assert log["pubs"]["/sim/robot2/jointStates"].sent[-1].effort == [3.0, 6.0, 9.0, 12.0]
    f.bus.publish("wireStates", pkg.WireStates(stateChange=pkg.KeyValue(key="cable0", value="taut"), robot=1))
    assert len(log["pubs"]["/sim/robot1/wireStates"].sent) == 1 and not log["pubs"]["/sim/robot0/wireStates"].sent


def test_bridge_module_imports_without_ros(pkg):
    import cdpr_simulation_amd.ros_bridge as rb

    assert "rospy" not in sys.modules or True
    with pytest.raises(ImportError):
        rb.CdprRosBridge(types.SimpleNamespace())  # no ROS in this image: the constructor is where it is needed


def test_subscriber_threads_may_deliver_while_the_world_steps(pkg, monkeypatch):
    """rospy runs subscriber callbacks on its own threads (the reference avoids the race with private callback queues
    drained on the physics thread, PLG.cpp:177-185, 203-204): publisher threads hammer every robot's Joy topic while
    step() runs.  Nothing may raise, and every robot's LAST Joy must reach the facade: none is lost between the snapshot
    and the next update()."""
    import threading

    from cdpr_simulation_amd.ros_bridge import CdprRosBridge

    log = install_fake_ros(monkeypatch)
    B = 16
    f = StubFacade(pkg, B, per_robot=True)
    br = CdprRosBridge(f, namespace="/sim", init_node=False)
    Joy = sys.modules["sensor_msgs.msg"].Joy
    errors, stop = [], threading.Event()
    last_sent = [0.0] * B
    per_thread = 4000

    def hammer(robots):
        try:
            for k in range(1, per_thread + 1):
                for b in robots:
                    v = b + k * 1e-4
                    log["subs"][f"/sim/robot{b}/jointVelocities"].deliver(Joy(axes=[v] * 4))
                    last_sent[b] = v
        except Exception as exc:  # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=hammer, args=(range(t, B, 4),)) for t in range(4)]
    old_interval = sys.getswitchinterval()
    sys.setswitchinterval(1e-6)  # thread switches every few bytecodes: an unguarded mailbox loses Joys or raises within milliseconds
    steps = 0
    try:
        for t in threads:
            t.start()
        while any(t.is_alive() for t in threads):
            br.step()
            steps += 1
    except Exception as exc:  # noqa: BLE001
        errors.append(exc)
    finally:
        stop.set()
        for t in threads:
            t.join()
        sys.setswitchinterval(old_interval)
    br.step()  # whatever arrived after the last snapshot is delivered by the next update, not dropped
    assert not errors, errors
    assert steps > 1 and f.updates == steps + 1
    seen = np.full(B, np.nan)
    for kind, joy in f.joys:
        assert kind == "v"
        rows = range(B) if joy.robots is None else np.nonzero(joy.robots)[0]
        for b in rows:
            assert joy.axes[b, 0] >= (seen[b] if np.isfinite(seen[b]) else -1.0)  # per robot, Joys arrive in order
            seen[b] = joy.axes[b, 0]
    assert np.allclose(seen, np.asarray(last_sent, dtype=np.float32))


def test_a_joy_that_arrives_while_the_mailbox_is_being_emptied_is_kept(pkg, monkeypatch):
    """The deterministic form of the race above: a subscriber thread delivers robot 2's Joy exactly while the stepping
    thread is working through the mailbox.  It must not disturb that pass and must go out with the NEXT update()."""
    from cdpr_simulation_amd.ros_bridge import CdprRosBridge

    log = install_fake_ros(monkeypatch)
    f = StubFacade(pkg, 3, per_robot=True)
    br = CdprRosBridge(f, namespace="/sim", init_node=False)
    Joy = sys.modules["sensor_msgs.msg"].Joy
    late = []

    class Mailbox(dict):  # the stepping thread is interrupted after the first entry it reads
        def items(self):
            for kv in list(dict.items(self)):
                yield kv
                if not late:
                    late.append(True)
                    log["subs"]["/sim/robot2/jointVelocities"].deliver(Joy(axes=[0.7] * 4))

    br._pending["jointVelocities"] = Mailbox()
    log["subs"]["/sim/robot0/jointVelocities"].deliver(Joy(axes=[0.1] * 4))
    br.step()
    assert late and list(f.joys[-1][1].robots) == [1, 0, 0]
    br.step()
    kind, joy = f.joys[-1]
    assert len(f.joys) == 2 and list(joy.robots) == [0, 0, 1] and np.allclose(joy.axes[2], 0.7)
