from byzpy_amd.engine.peer_to_peer.topology import Topology
from byzpy_amd.engine.peer_to_peer.train import PeerToPeer
from byzpy_amd.engine.peer_to_peer.gossip import gossip_round

__all__ = ["Topology", "PeerToPeer", "gossip_round"]
